"""Residuals, pose information and the LM polish under the depth mask on the device (csrc/pcl_depth_info.hip).

Scenes, cases and the float64 composition: tests/depth_info_helpers.py (depth_helpers' occluder scene, 33,768 points = 8 x 4096 + 1000, its
three poses, the cases W1 / W4 / W7 / C1 and two tiny clouds of 513 and 700 points on a 16 x 32 grid; a 128 x 256 panorama as F32, U8 and
F16 texels; B = 3 and B = 2).  What is asserted, in the order of the tests:
 1. the `visible` row equals depth_helpers.expected_visible on every point the model can decide, against the device's own z-buffer;
 2. a visible point's residual is the plain row's bit for bit, a hidden one's exactly -1;
 3. with a tolerance that hides nothing every output of the three ops equals the plain op's bit for bit, both objectives;
 4. the info record lies inside the propagated per-point bounds of the float64 model under the device's own visible row, M exactly;
 5. the LM chain's trace is the algorithm on pose_information(depth=...) at its own trial poses, bit for bit;
 6. results do not depend on what the workspaces held, guards intact;
 7. omniloc_batch with cfg.depth_polish."""
import numpy as np
import pytest

import depth_helpers as dh
import depth_info_helpers as dih
import gn_helpers as gn
import info_helpers as ih
import ws_helpers as ws
from conftest import Cfg

gpu = pytest.mark.gpu
FMTS = ("f32", "u8", "f16")
ITERS = 6


@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CLOUDS, _PANOS = {}, {}


def _cloud(ops, oracle, case):
    """-> (cloud, order: packed slot -> point of the scene)"""
    if case not in _CLOUDS:
        xyz, rgb = dih.scene(oracle)[:2]
        x, c = dih.case_points(case, xyz, rgb)
        cloud = ops.Cloud(T(x), T(c), sort=True)
        _CLOUDS[case] = (cloud, cloud.order.cpu().numpy())
    return _CLOUDS[case]


def _pano(ops, oracle, fmt):
    if fmt not in _PANOS:
        _PANOS[fmt] = ops.Pano(T(dih.scene(oracle)[2]), fmt=fmt)
    return _PANOS[fmt]


def _bits(t):
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    import torch
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _rows(out):
    H, b, st, cov = (t.cpu().numpy().astype(np.float64) for t in out)
    return [dict(H=H[i], b=b[i], M=st[i, 0], S1=st[i, 1], S2=st[i, 2], sigma2=st[i, 3], status=st[i, 4], cov=cov[i]) for i in range(len(H))]


# ------------------------------------------------------------------------------------------------ 1, 2: visibility and residual values
@gpu
@pytest.mark.parametrize("case", list(dih.CASES))
def test_visible_rows_and_residual_values(ops, oracle, parity, case):
    """1. Z: the device's z-buffers of pcl_depth_mask at the same poses, grid, tolerance and stride (the same pcl_launch_zbuffers; a
    min-reduction is order-free).  On every point expected_visible decides, `visible` equals it exactly; the undecided share stays under
    LEFT_OUT_CAP; packed and caller order agree through the cloud's order; B = 3 and B = 2 give the same rows.
    2. For every texel format: where visible is 1 the row equals plain point_residuals bit for bit, where it is 0 it is exactly -1."""
    xyz, rgb, img, trans, rot = dih.scene(oracle)
    cloud, order = _cloud(ops, oracle, case)
    _, grid, stride, tau = dih.CASES[case]
    kw = dih.depth_kw(case)
    cm = dih.case_model(oracle, case, order)
    z, _ = dh.run_depth_mask(ops, cloud, trans, rot, grid, tau, stride)
    rule = [dh.expected_visible(cm, b, z[b]) for b in range(dh.B_POSES)]
    left_out = max(1.0 - float(decided.mean()) for _, decided in rule)
    for fmt in FMTS:
        pano = _pano(ops, oracle, fmt)
        res_p, vis_p = ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True, depth=kw, return_visible=True)
        res_c, vis_c = ops.point_residuals(cloud, pano, T(trans), T(rot), depth=kw, return_visible=True)
        plain_p = ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True)
        only = ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True, depth=kw)
        assert _same(only, res_p)
        res2, vis2 = ops.point_residuals(cloud, pano, T(trans[:2]), T(rot[:2]), packed=True, depth=kw, return_visible=True)
        assert _same(res2, res_p[:2]) and _same(vis2, vis_p[:2]), (case, fmt)
        vp, vc = vis_p.cpu().numpy(), vis_c.cpu().numpy()
        rp, rc, pl = (t.cpu().numpy().view(np.uint32) for t in (res_p, res_c, plain_p))
        assert vp.dtype == np.uint8 and set(np.unique(vp)) <= {0, 1}
        minus_one = np.float32(-1).view(np.uint32)
        for b in range(dh.B_POSES):
            # caller order = packed order through `order`
            assert np.array_equal(vc[b][order], vp[b]) and np.array_equal(rc[b][order], rp[b]), (case, fmt, b)
            expect, decided = rule[b]
            wrong = np.nonzero(decided & (vp[b].astype(bool) != expect))[0]
            assert len(wrong) == 0, "%s %s pose %d: %d decided points with the wrong visibility, first packed slots %s" % (case, fmt, b, len(wrong),
                                                                                                                     wrong[:8])
            if dih.CASES[case][0] is None:
                assert expect[decided].any() and not expect[decided].all()          # the z-buffer hides something, and not everything
            seen = vp[b] == 1
            assert np.array_equal(rp[b][seen], pl[b][seen]), (case, fmt, b)
            assert (rp[b][~seen] == minus_one).all(), (case, fmt, b)
    parity("%s: points left out of the visibility check (border + threshold ties, worst pose)" % case, left_out, dh.LEFT_OUT_CAP)
    assert left_out <= dh.LEFT_OUT_CAP


# ------------------------------------------------------------------------------------------------ 3: nothing hidden => the plain result
@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", ["W1", "W4", "C1", "t700"])
def test_nothing_hidden_is_the_plain_result(ops, oracle, case, fmt):
    """depth_tau = 1e6: every point passes the test, every cell is +inf or huge — residuals, the info record (H, b, stats, cov) and the
    chain (every trace row, every output) equal the plain calls bit for bit, for L2 and L1, B = 3 and B = 2"""
    _, _, _, trans, rot = dih.scene(oracle)
    cloud, _ = _cloud(ops, oracle, case)
    pano = _pano(ops, oracle, fmt)
    kw = dict(dih.depth_kw(case), depth_tau=dih.NOTHING_HIDDEN_TAU)
    for B in (3, 2):
        tr, ro = T(trans[:B]), T(rot[:B])
        res, vis = ops.point_residuals(cloud, pano, tr, ro, depth=kw, return_visible=True)
        assert bool((vis == 1).all()) and _same(res, ops.point_residuals(cloud, pano, tr, ro)), (case, fmt, B)
        for obj in (dict(), dict(objective="l1"), dict(objective="l1", delta=1.0 / 255)):
            plain, masked = ops.pose_information(cloud, pano, tr, ro, **obj), ops.pose_information(cloud, pano, tr, ro, depth=kw, **obj)
            assert all(_same(a, b) for a, b in zip(plain, masked)), (case, fmt, B, obj)
            p = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=ITERS, trace=True, **obj)
            m = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=ITERS, trace=True, depth=kw, **obj)
            assert set(p) == set(m)
            for key in p:
                assert _same(p[key], m[key]), (case, fmt, B, obj, key)
            assert float(p["accepted"].min()) >= 1


# ------------------------------------------------------------------------------------------------ 4: the sums under the mask
@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", list(dih.CASES))
def test_sums_under_the_mask_against_the_model(ops, oracle, parity, case, fmt):
    """The record of each pose against depth_info_helpers' float64 sums with the device's own `visible` row as 0/1 weights (test 1 has proven
    that row on every decidable point): M = the count of visible, non-black points exactly (the device's own rows), S1, S2, sigma^2 and
    every entry of H and b inside depth_info_helpers.bounds, cov inside info_helpers.cov_bound (info_helpers.violations finds nothing),
    status 0.  B = 3 in one call; B = 2 gives the first two records bit for bit."""
    _, _, _, trans, rot = dih.scene(oracle)
    cloud, order = _cloud(ops, oracle, case)
    pano = _pano(ops, oracle, fmt)
    kw = dih.depth_kw(case)
    out = ops.pose_information(cloud, pano, T(trans), T(rot), depth=kw)
    two = ops.pose_information(cloud, pano, T(trans[:2]), T(rot[:2]), depth=kw)
    assert all(_same(a[:2], b) for a, b in zip(out, two)), (case, fmt)
    res, vis = ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True, depth=kw, return_visible=True)
    res, vis = res.cpu().numpy(), vis.cpu().numpy().astype(bool)
    for b, g in enumerate(_rows(out)):
        m64, m32 = (dih.take(m, order) for m in dih.point_models(oracle, b))
        bd = dih.bounds(m64, m32, vis[b])
        tag = "%s %s pose %d" % (case, fmt, b)
        count = int((vis[b] & (res[b] != -1.0)).sum())
        assert np.isfinite(res[b]).all() and g["M"] == count, (tag, g["M"], count)
        assert bd["undecided_kept"] == 0, (tag, bd["undecided_kept"])
        assert g["status"] == 0, tag
        ref = bd["ref"]
        nH = np.sqrt(np.outer(np.diag(ref["H"]), np.diag(ref["H"])))
        parity(tag + ": masked H, worst entry, / sqrt(H_kk H_ll)", (np.abs(g["H"] - ref["H"]) / nH).max(), (bd["BH"] / nH).max(),
               (np.abs(bd["yard"]["H"] - ref["H"]) / nH).max())
        print("%s: M %d of %d visible of %d; H %.3e b %.3e S1 %.3e S2 %.3e sigma2 %.3e of their bounds; border share %.2e"
              % (tag, g["M"], vis[b].sum(), len(order), (np.abs(g["H"] - ref["H"]) / bd["BH"]).max(), (np.abs(g["b"] - ref["b"]) / bd["Bb"]).max(),
                 abs(g["S1"] - ref["S1"]) / bd["BS1"], abs(g["S2"] - ref["S2"]) / bd["BS2"], abs(g["sigma2"] - ref["sigma2"]) / bd["Bsig"],
                 bd["border_share"]))
        assert ih.violations(g, bd) == [], tag


# ------------------------------------------------------------------------------------------------ 5: the LM chain under the mask
def _runs(res):
    host = {key: v.cpu().numpy() for key, v in res.items() if v is not None}
    out = []
    for i in range(host["trans"].shape[0]):
        r = dict(theta=np.concatenate([host["trans"][i], host["rot"][i]]), trace=host["trace"][:, i])
        for key in ("sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats", "cov"):
            r[key] = host[key][i] if key in host else None
        out.append(r)
    return out


def _info_at(ops, cloud, pano, thetas, kw, obj):
    """ops.pose_information(depth=...) at every pose of thetas in ONE call, and the residual / visible rows there -> lookup by theta"""
    uniq = {np.asarray(t, np.float32).tobytes(): np.asarray(t, np.float32) for t in thetas}
    th = np.stack(list(uniq.values()))
    tr, ro = T(th[:, :3].copy()), T(th[:, 3:].copy())
    out = ops.pose_information(cloud, pano, tr, ro, depth=kw, **obj)
    H, b, st = (t.cpu().numpy() for t in out[:3])
    cov = None if out[3] is None else out[3].cpu().numpy()
    res, vis = ops.point_residuals(cloud, pano, tr, ro, packed=True, depth=kw, return_visible=True)
    count = ((vis == 1) & (res != -1.0)).sum(1).cpu().numpy()
    table = {key: dict(F=st[i, 3], M=st[i, 0], ok=st[i, 4] != 1, H=H[i].astype(np.float64), b=b[i].astype(np.float64), H32=H[i], b32=b[i], stats=st[i],
                       cov=None if cov is None else cov[i], count=int(count[i])) for i, key in enumerate(uniq)}
    return lambda theta: table[np.asarray(theta, np.float32).tobytes()]


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", ["W1", "W4", "W7", "C1", "t513", "t700"])
def test_the_chain_under_the_mask_is_the_algorithm(ops, oracle, parity, case, fmt):
    """iters = 6 from case_poses(), both objectives: at every evaluation's trial pose F and M of the trace equal pose_information(depth=...)
    there bit for bit (the same kernels' arithmetic on z-buffers rebuilt at that pose), M is the count of visible non-black points of
    point_residuals(depth=..., return_visible=True) there, the accept / reject / lambda sequence, the counters, the returned pose and every
    step satisfy gn_helpers.trace_violations with that evaluator, the final record (and cov) is pose_information(depth=...) at the returned
    pose bit for bit, and the returned sigma^2 is at most the starting one in fp32.  B = 2 gives the first two poses' bits."""
    _, _, _, trans, rot = dih.scene(oracle)
    cloud, _ = _cloud(ops, oracle, case)
    pano = _pano(ops, oracle, fmt)
    kw = dih.depth_kw(case)
    h = gn.hyper()
    for obj in (dict(), dict(objective="l1")):
        res = ops.gauss_newton_refine(cloud, pano, T(trans), T(rot), iters=ITERS, trace=True, depth=kw, **obj)
        two = ops.gauss_newton_refine(cloud, pano, T(trans[:2]), T(rot[:2]), iters=ITERS, trace=True, depth=kw, **obj)
        for key in res:
            a = res[key][:, :2] if key == "trace" else (None if res[key] is None else res[key][:2])
            assert _same(a, two[key]), (case, fmt, obj, key)
        runs = _runs(res)
        at = _info_at(ops, cloud, pano, np.concatenate([r["trace"][: int(r["evaluations"]), :6] for r in runs] + [r["theta"][None] for r in runs]), kw, obj)
        for b, r in enumerate(runs):
            tag = "%s %s %s pose %d" % (case, fmt, obj.get("objective", "l2"), b)
            worst = []
            bad = gn.trace_violations(r, h, ITERS, at, report=lambda a, bnd: worst.append((a, bnd)))
            assert bad == [], (tag, bad)
            if worst:
                parity(tag + ": worst step against the float64 solve", worst[0][0], worst[0][1])
            for k in range(int(r["evaluations"])):
                e = at(r["trace"][k, :6])
                assert float(e["M"]) == e["count"], (tag, k, e["M"], e["count"])
            fin = at(r["theta"])
            assert _eq(r["H"], fin["H32"]) and _eq(r["b"], fin["b32"]) and _eq(r["stats"], fin["stats"]) and _eq(r["cov"], fin["cov"]), tag
            assert int(r["status"]) in (0, 3) and np.float32(r["sigma2"]) <= np.float32(r["sigma2_start"]), (tag, r["status"], r["sigma2"], r["sigma2_start"])
            print("%s: F %.6g -> %.6g, %d accepted, %d rejected, status %d" % (tag, r["sigma2_start"], r["sigma2"], r["accepted"], r["rejected"], r["status"]))


# ------------------------------------------------------------------------------------------------ 6: the memory contract
def _contract_scenario(oracle, case, fmt):
    def scenario():
        from piccolo_amd import ops
        xyz, rgb, img, trans, rot = dih.scene(oracle)
        x, c = dih.case_points(case, xyz, rgb)
        cloud, pano = ops.Cloud(T(x), T(c), sort=True), ops.Pano(T(img), fmt=fmt)
        kw = dih.depth_kw(case)
        out = {}
        out["res"], out["vis"] = ops.point_residuals(cloud, pano, T(trans), T(rot), depth=kw, return_visible=True)
        out["res_packed"] = ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True, depth=kw)
        out["info"] = ops.pose_information(cloud, pano, T(trans), T(rot), depth=kw)
        out["info_l1"] = ops.pose_information(cloud, pano, T(trans), T(rot), depth=kw, objective="l1")
        out["gn"] = ops.gauss_newton_refine(cloud, pano, T(trans), T(rot), iters=3, trace=True, depth=kw)
        out["gn_l1"] = ops.gauss_newton_refine(cloud, pano, T(trans[:2]), T(rot[:2]), iters=2, trace=True, depth=kw, objective="l1")
        return ws.flat(out)
    return scenario


@gpu
@pytest.mark.parametrize("case,fmt", [("W4", "f16"), ("C1", "u8"), ("t700", "f32")])
def test_results_do_not_depend_on_what_the_workspaces_held(oracle, case, fmt):
    """the three ops on caller-poisoned workspaces, states and outputs with the three fill words of ws_helpers: identical results across
    the fills and the unpatched run, guard bytes on both sides of every workspace and output untouched, the same allocations each time"""
    scenario = _contract_scenario(oracle, case, fmt)
    ref = scenario()
    runs = ws.poisoned_runs(scenario)
    ws.assert_contract(ref, runs)
    callers = {c[0] for _, c in runs[ws.FILL_WORDS[0]].callers}
    assert {"_point_residuals_depth", "_pose_information", "_gauss_newton"} <= callers, callers


# ------------------------------------------------------------------------------------------------ 7: omniloc_batch with cfg.depth_polish
@gpu
def test_omniloc_batch_with_depth_polish(ops, oracle):
    """The scene of test_depth_mask_vs_oracle_and_in_the_gd_loop (40,000 points, 128 x 256, B = 4, 60 iterations).  Without the key the
    three entries are those of today's depth chain; with gn_iters = 5, t, R and cov equal a manual gauss_newton_refine_at_winners(depth=...)
    from the same engine's winners row bit for bit and the loss is ops.sampling_loss(depth=...)[0] at that pose; with gn_lambda so large
    that no step is accepted the chain's own entries come back; pose_covariance alone appends a fourth entry and leaves the three."""
    import torch
    from piccolo_amd import omniloc as po
    from piccolo_amd import synth
    H, W, B = 128, 256, 4
    xyz, rgb = dh.occluder_scene(40_000)                        # (test_hip_parity._occluder_scene(40_000): that test's scene, point for point)
    n = len(xyz)
    t_gt, ypr_gt = synth.gt_pose(17)
    trans, rot = synth.start_poses(t_gt, ypr_gt, B, seed=17, sigma_t=0.1, sigma_r=0.05)
    img = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (H, W)).astype(np.float32) / 255
    base = dict(lr=0.1, num_iter=60, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B, depth_mask=True)
    X, C, I = T(xyz), T(rgb), T(img)

    def run(**keys):
        return po.omniloc_batch(I, X, C, T(trans.copy()), T(rot.copy()), Cfg(**base, **keys), {})
    chain = run()
    assert len(chain) == 3
    again = run(depth_polish=False)
    assert all(torch.equal(a, b) for a, b in zip(chain, again))
    # the manual polish from the same engine's winners row
    cfg = Cfg(**base, depth_polish=True, gn_iters=5)
    cloud, pano = po.packed_cloud(X, C), po.packed_pano(I, n_points=n)
    gd = po._refine(X, C, [pano], T(trans.copy()), T(rot.copy()), po.quantile_box_of(X, 0.05), cfg, True)
    win = gd.winner(1, *po._leaf_buffers(T(trans.copy()), T(rot.copy()), gd.B)[:2]).clone()
    depth = po._depth_cfg(cfg)
    manual = ops.gauss_newton_refine_at_winners(cloud, pano, win, iters=5, depth=depth)
    assert int(manual["accepted"][0]) > 1 and int(manual["status"][0]) in (0, 3)          # the polish takes a step on this scene
    polished = run(depth_polish=True, gn_iters=5, pose_covariance=True)
    assert len(polished) == 4
    assert _same(polished[0], manual["trans"][0].reshape(3, 1).cpu())
    assert _same(polished[1], ops.rot_from_ypr(manual["rot"])[0].reshape(3, 3).cpu())
    assert _same(polished[3], manual["cov"][0].cpu())
    loss = ops.sampling_loss(cloud, pano, manual["trans"], manual["rot"], with_grad=False, depth=depth)[0, 0].cpu()
    assert _same(polished[2], loss)
    three = run(depth_polish=True, gn_iters=5)
    assert len(three) == 3 and all(_same(a, b) for a, b in zip(three, polished[:3]))
    # no step accepted: the chain's own entries, bit for bit
    stuck = run(depth_polish=True, gn_iters=5, gn_lambda=1e30)
    assert len(stuck) == 3 and all(_same(a, b) for a, b in zip(stuck, chain))
    # the covariance alone: a fourth entry, the first three unchanged; it is pose_information(depth=...) at the winner
    with_cov = run(depth_polish=True, pose_covariance=True)
    assert len(with_cov) == 4 and all(_same(a, b) for a, b in zip(with_cov[:3], chain))
    assert _same(with_cov[3], ops.pose_information_at_winners(cloud, pano, win, depth=depth)[3][0].cpu())
    assert bool(torch.isfinite(with_cov[3]).all()) and bool(torch.isfinite(polished[3]).all())
