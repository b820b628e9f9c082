"""GPU tests of the per-point residuals (pcl_point_residuals), the robust weight plane made from them (pcl_robust_weights) and the robust
re-weighted refinement chain (cfg.robust_iters of omniloc_batch).  Build-defined: the reference has neither.

Scenes as in test_point_weights.py: S1 = 1025 points on 32 x 64 (three steps, a ragged last one), S2 = 50,001 points on 64 x 128, S3 = S2's
points on 128 x 256 with 20 % of the cloud's colours replaced by uniform random ones after the render."""
import numpy as np
import pytest
import torch

from conftest import Cfg
from parity_helpers import T, rel

pytestmark = pytest.mark.gpu

FMTS = ("f16", "u8", "f32")
SHAPES = {"S1": (1025, 32, 64), "S2": (50001, 64, 128), "S3": (50001, 128, 256)}
CASES = [("S1", 3), ("S1", 4), ("S2", 4)]


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


_SCENES, _DEVICE, _COMP = {}, {}, {}


def scene(oracle, name):
    """(xyz, rgb, img, t_gt, ypr_gt) of a shape, computed once and shared; S3: rgb recoloured after the render, plus (rgb0, hit)"""
    if name not in _SCENES:
        from piccolo_amd import synth
        n, H, W = SHAPES[name]
        xyz, rgb = synth.box_room(n, seed=n % 89)
        t_gt, ypr_gt = synth.gt_pose(n % 97)
        img = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (H, W)).astype(np.float32) / 255
        extra = ()
        if name == "S3":
            rng = np.random.default_rng(5)
            hit = rng.random(n) < 0.2
            rgb0, rgb = rgb, rgb.copy()
            rgb[hit] = rng.random((int(hit.sum()), 3)).astype(np.float32)
            extra = (rgb0, hit)
        _SCENES[name] = (xyz, rgb, img, np.asarray(t_gt, np.float32), np.asarray(ypr_gt, np.float32)) + extra
    return _SCENES[name]


def poses(oracle, name, B):
    from piccolo_amd import synth
    xyz, _, _, t_gt, ypr_gt = scene(oracle, name)[:5]
    return synth.start_poses(t_gt, ypr_gt, B, seed=xyz.shape[0])


def device_case(ops, oracle, name, B, fmt):
    """cloud, panorama, poses and both residual tensors of a case, computed once"""
    key = (name, B, fmt)
    if key not in _DEVICE:
        xyz, rgb, img = scene(oracle, name)[:3]
        trans, rot = poses(oracle, name, B)
        cloud, pano = ops.Cloud(T(xyz), T(rgb)), ops.Pano(T(img), fmt=fmt)
        _DEVICE[key] = dict(cloud=cloud, pano=pano, trans=trans, rot=rot, caller=ops.point_residuals(cloud, pano, T(trans), T(rot)),
                            packed=ops.point_residuals(cloud, pano, T(trans), T(rot), packed=True))
    return _DEVICE[key]


def compose(oracle, xyz, rgb, img, t, ypr, dtype):
    """the reference's formulas, one pose: rot_from_ypr, (x - t) R^T, cloud2idx, sample_from_img, norm -> (residual (n,), kept (n,))"""
    x, c0, t = np.asarray(xyz, dtype), np.asarray(rgb, dtype), np.asarray(t, dtype).reshape(1, 3)
    R = oracle.rot_from_ypr(ypr, dtype).astype(dtype)
    p = (x - t) @ R.T
    c = oracle.sample_from_img(np.asarray(img, dtype), oracle.cloud2idx(p, dtype), dtype)
    d = c - c0
    return np.sqrt((d * d).sum(1)), (c != 0).any(1)


def composed(oracle, name, B):
    """per pose the fp64 and fp32 compositions of a case, computed once"""
    key = (name, B)
    if key not in _COMP:
        xyz, rgb, img = scene(oracle, name)[:3]
        trans, rot = poses(oracle, name, B)
        _COMP[key] = [(compose(oracle, xyz, rgb, img, trans[b], rot[b], np.float64), compose(oracle, xyz, rgb, img, trans[b], rot[b], np.float32))
                      for b in range(B)]
    return _COMP[key]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,B", CASES)
def test_same_mask_and_same_sum_as_the_loss_kernel(ops, oracle, parity, name, B, fmt):
    """(row >= 0).sum() is the loss kernel's count exactly; the fp64 mean of the kept entries is its loss up to the summation order: within 3 x
    the loss kernel's own distance from the fp64 oracle"""
    d = device_case(ops, oracle, name, B, fmt)
    xyz, rgb, img = scene(oracle, name)[:3]
    out = ops.sampling_loss(d["cloud"], d["pano"], T(d["trans"]), T(d["rot"]), with_grad=False)
    res = d["caller"]
    kept = res >= 0
    assert torch.equal(kept.sum(1).to(torch.float32), out[:, 1]), (kept.sum(1), out[:, 1])
    assert ((res == -1) | kept).all()
    mean = (torch.where(kept, res, torch.zeros_like(res)).double().sum(1) / kept.sum(1).double()).cpu().numpy()
    loss = out[:, 0].cpu().numpy()
    r64 = oracle.sampling_loss(xyz, rgb, img, d["trans"], d["rot"], dtype=np.float64, grad=False)
    own = rel(loss, r64["loss"])
    got = rel(mean, loss)
    print("%s B=%d %s: loss kernel vs fp64 %.3e, residual mean vs loss kernel %.3e" % (name, B, fmt, own, got))
    dcount = float(np.abs(out[:, 1].cpu().numpy() - r64["count"]).max())
    parity("loss kernel vs fp64", own, 3e-7 + 2.0 * dcount / xyz.shape[0])
    parity("residual mean vs loss kernel", got, 3 * own, own)


@pytest.mark.parametrize("name,B", CASES)
def test_same_values_across_orders_strides_and_formats(ops, oracle, name, B):
    rows = {}
    for fmt in FMTS:
        d = device_case(ops, oracle, name, B, fmt)
        cloud, pano = d["cloud"], d["pano"]
        n = cloud.n
        # caller order == packed order gathered through the cloud's order
        back = torch.empty_like(d["packed"])
        back[:, cloud.order] = d["packed"]
        assert same_bits(d["caller"], back), fmt
        # pose stride 16 on a winners-shaped tensor == pose stride 3 on the same poses
        win = torch.full((B, 16), float("nan"), device="cuda")
        win[:, 0:3], win[:, 13:16] = T(d["trans"]), T(d["rot"])
        assert same_bits(ops.point_residuals_at_winners(cloud, pano, win), d["caller"]), fmt
        assert same_bits(ops.point_residuals_at_winners(cloud, pano, win, packed=True), d["packed"]), fmt
        # an unsorted cloud: its packed order is the caller's
        plain = ops.Cloud(cloud.xyz, T(scene(oracle, name)[1]), sort=False)
        assert plain.order is None and same_bits(ops.point_residuals(plain, pano, T(d["trans"]), T(d["rot"])), d["caller"]), fmt
        rows[fmt] = d["caller"]
        assert d["caller"].shape == (B, n)
    assert same_bits(rows["u8"], rows["f16"])


def head_case(ops, oracle, n, B):
    """the first n points of S1 against S1's u8 panorama under B of its start poses"""
    xyz, rgb, img = scene(oracle, "S1")[:3]
    trans, rot = poses(oracle, "S1", B)
    return ops.Cloud(T(xyz[:n]), T(rgb[:n])), ops.Pano(T(img), fmt="u8"), T(trans), T(rot)


@pytest.mark.parametrize("packed", [True, False])
def test_more_poses_on_one_panorama_than_an_address_list_holds(ops, oracle, packed):
    """B = 65 poses on ONE panorama, n = 513 (two steps, the second one point): one call == the 65 one-pose calls stacked, bit for bit.  The
    several-image form carries 64 panorama addresses per launch; the single form takes any B in one launch and must not go through that list."""
    cloud, pano, trans, rot = head_case(ops, oracle, 513, 65)
    got = ops.point_residuals(cloud, pano, trans, rot, packed=packed)
    assert got.shape == (65, 513)
    alone = torch.cat([ops.point_residuals(cloud, pano, trans[b:b + 1], rot[b:b + 1], packed=packed) for b in range(65)])
    assert same_bits(got, alone)
    assert (got >= 0).any() and (got == -1).any()             # (neither all kept nor all masked)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_the_residual_walk_is_the_information_walk(ops, oracle, n):
    """n where a pair, a step or a chunk is partial (the information kernel deals at least two steps to a chunk, the residual kernel one): per
    pose, the kept entries of point_residuals are counted by pose_information's M exactly, and their float64 sum is its S1.

    The bound is info_helpers.bounds' BS1 = n e + ADDS u S1 with e = 0: both kernels hold the SAME fp32 l_i per point (one body, the same
    instructions on the same inputs; the cloud has no weights), so what is left is the information kernel's ADDS fp32 roundings per sum."""
    import info_helpers as ih
    cloud, pano, trans, rot = head_case(ops, oracle, n, 3)
    res = ops.point_residuals(cloud, pano, trans, rot)
    stats = ops.pose_information(cloud, pano, trans, rot)[2].cpu().numpy().astype(np.float64)
    kept = res >= 0
    assert ((res == -1) | kept).all()
    assert np.array_equal(kept.sum(1).cpu().numpy().astype(np.float64), stats[:, 0]), (n, kept.sum(1), stats[:, 0])
    s1 = torch.where(kept, res, torch.zeros_like(res)).double().sum(1).cpu().numpy()
    bound = ih.ADDS * ih.U * s1
    print("n=%d: M %s; |S1 - sum| %s of bound %s" % (n, stats[:, 0], np.abs(stats[:, 1] - s1), bound))
    assert (np.abs(stats[:, 1] - s1) <= bound).all(), (n, stats[:, 1], s1)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,B", CASES)
def test_per_point_against_the_reference_formulas(ops, oracle, parity, name, B, fmt):
    """per point within 3 x the composition's own fp32-vs-fp64 gap (per case: the maximum over its points and poses); points whose masks
    differ between the precisions (or on the device) are left out, at most 0.1 % of them"""
    d = device_case(ops, oracle, name, B, fmt)
    res = d["caller"].cpu().numpy()
    n = res.shape[1]
    worst, gap_worst, left_out = 0.0, 0.0, 0
    for b, ((v64, k64), (v32, k32)) in enumerate(composed(oracle, name, B)):
        dev_kept = res[b] >= 0
        out = (k64 != k32) | (dev_kept != k64)
        left_out = max(left_out, int(out.sum()))
        both = k64 & ~out
        assert (res[b][~k64 & ~out] == -1).all()
        gap = float(np.abs(v32.astype(np.float64) - v64)[both].max())
        err = float(np.abs(res[b].astype(np.float64) - v64)[both].max())
        print("%s B=%d %s pose %d: device vs fp64 %.3e, fp32 vs fp64 %.3e, left out %d" % (name, B, fmt, b, err, gap, int(out.sum())))
        worst, gap_worst = max(worst, err), max(gap_worst, gap)
    parity("points with another mask", left_out, 1e-3 * n)
    parity("residual vs fp64 composition", worst, 3 * gap_worst, gap_worst)


def torch_weights(row, kind, k):
    """the definitions on the CPU from the device's own residual row (packed): (s, M, weights (n,))"""
    r = row.cpu()
    valid = r[r != -1]
    M = int(valid.numel())
    if M == 0:
        return torch.zeros(()), 0, torch.ones_like(r)
    s = torch.sort(valid).values[(M - 1) // 2]
    c = torch.tensor(k, dtype=torch.float32) * s
    inlier = r <= c
    if kind == "trunc":
        w = inlier.to(torch.float32)
    else:
        w = torch.where(inlier, torch.ones_like(r), c / r if not torch.isnan(c) else torch.zeros_like(r))
    w = torch.where(torch.isfinite(r), w, torch.zeros_like(r))
    return s, M, torch.where(r == -1, torch.ones_like(r), w)


def check_plane(ops, cloud, row, kind, k=2.5):
    plane, scale = ops.robust_weights(cloud, row, kind, k)
    s, M, w = torch_weights(row, kind, k)
    n, sc = cloud.n, scale.cpu()
    assert plane.numel() == ops._lib.load().pcl_cloud_stride(n) and (plane[n:] == 0).all()
    assert float(sc[1]) == M
    assert (torch.isnan(sc[0]) and torch.isnan(s)) or same_bits(sc[0:1], s.reshape(1)), (sc, s)
    assert not torch.isnan(plane).any()
    assert same_bits(plane[:n].cpu(), w), (kind, (bits(plane[:n].cpu()) != bits(w)).sum())
    return plane, sc


@pytest.mark.parametrize("kind", ["trunc", "huber"])
@pytest.mark.parametrize("name,B", [("S1", 3), ("S2", 4)])
def test_select_and_weights_against_torch(ops, oracle, name, B, kind):
    """s, M and the plane, bit for bit against a CPU sort of the device's own row (masked slots 1, padding 0)"""
    d = device_case(ops, oracle, name, B, "f16")
    n = d["cloud"].n
    for b in range(B):
        row = d["packed"][b]
        for k in (2.5, 1.0, 0.5):
            plane, sc = check_plane(ops, d["cloud"], row, kind, k)
            assert 0 < float(sc[1]) <= n and float(sc[0]) > 0
            assert (plane[:n][row == -1] == 1).all()
            if k <= 1.0:                                   # a threshold at or below the median: the upper half is cut
                assert ((plane[:n] == 0) if kind == "trunc" else ((plane[:n] > 0) & (plane[:n] < 1))).sum() > n // 4
    # in place: the same plane tensor is written again
    again, _ = ops.robust_weights(d["cloud"], d["packed"][0], kind, 2.5, plane=plane)
    assert again is plane and same_bits(plane[:n].cpu(), torch_weights(d["packed"][0], kind, 2.5)[2])


@pytest.mark.parametrize("kind", ["trunc", "huber"])
def test_select_and_weights_edge_cases(ops, oracle, kind):
    xyz, rgb, img = scene(oracle, "S1")[:3]
    trans, rot = poses(oracle, "S1", 3)
    n = xyz.shape[0]
    cloud = ops.Cloud(T(xyz), T(rgb))
    # an all-black panorama: every point masked, M = 0, the unit plane
    row = ops.point_residuals(cloud, ops.Pano(torch.zeros(32, 64, 3).cuda(), fmt="f16"), T(trans[:1]), T(rot[:1]), packed=True)[0]
    assert (row == -1).all()
    plane, sc = check_plane(ops, cloud, row, kind)
    assert (plane[:n] == 1).all() and float(sc[0]) == 0 and float(sc[1]) == 0
    # a one-colour cloud on a one-colour panorama: 1025 tied residuals
    flat = ops.Cloud(T(xyz), torch.full((n, 3), 0.25).cuda())
    grey = ops.Pano((torch.full((32, 64, 3), 128.0) / 255).cuda(), fmt="f16")
    row = ops.point_residuals(flat, grey, T(trans[:1]), T(rot[:1]), packed=True)[0]
    # (the points of the +-0.99 strip blend with the zero border: every other point samples the one colour)
    kept = row[row != -1]
    tie = kept.median()
    assert kept.numel() > n // 2 and (bits(kept) == bits(tie.reshape(1))).sum() > 0.9 * n
    plane, sc = check_plane(ops, flat, row, kind)
    assert same_bits(sc[0:1], tie.reshape(1).cpu())
    # ... and all 1025 tied
    row = torch.full((n,), float(tie), device="cuda")
    plane, sc = check_plane(ops, flat, row, kind)
    assert (plane[:n] == 1).all() and same_bits(sc[0:1], row[:1].cpu()) and float(sc[1]) == n
    plane, sc = check_plane(ops, flat, row, kind, k=0.999)
    assert ((plane[:n] == 0) if kind == "trunc" else ((plane[:n] > 0.99) & (plane[:n] < 1))).all()
    # n = 1
    one = ops.Cloud(T(xyz[:1]), T(rgb[:1]))
    row = ops.point_residuals(one, ops.Pano(T(img), fmt="f16"), T(trans[:1]), T(rot[:1]), packed=True)[0]
    plane, sc = check_plane(ops, one, row, kind)
    assert plane.numel() == 256 and float(plane[0]) == 1
    # a pose with a NaN: the row is NaN, the weights 0, no NaN in the plane
    bad = trans[:1].copy()
    bad[0, 1] = np.nan
    row = ops.point_residuals(cloud, ops.Pano(T(img), fmt="f16"), T(bad), T(rot[:1]), packed=True)[0]
    assert torch.isnan(row).all()
    plane, sc = check_plane(ops, cloud, row, kind)
    assert (plane == 0).all() and torch.isnan(sc[0]) and float(sc[1]) == n


def test_recoloured_points_lose_their_vote(ops, oracle, parity):
    """S3 at the ground-truth pose, TRUNC, k = 2.5, through the omniloc surface (the caller's point order)"""
    from piccolo_amd import omniloc as po
    xyz, rgb, img, t_gt, ypr_gt, rgb0, hit = scene(oracle, "S3")
    n = xyz.shape[0]
    x, c, im = T(xyz), T(rgb), T(img)
    res = po.point_residuals(im, x, c, T(t_gt.reshape(1, 3)), T(ypr_gt.reshape(1, 3)))
    assert res.shape == (1, n)
    w = po.robust_weights(res[0], kind="trunc", k=2.5)
    assert w.shape == (n,) and set(w.unique().tolist()) <= {0.0, 1.0}
    # the surface's weights are the packed plane's, point by point
    cloud = po.packed_cloud(x, c)
    row = ops.point_residuals(cloud, po.packed_pano(im, n_points=n), T(t_gt.reshape(1, 3)), T(ypr_gt.reshape(1, 3)), packed=True)[0]
    plane, scale = ops.robust_weights(cloud, row, "trunc", 2.5)
    assert same_bits(w[cloud.order], plane[:n]) and cloud.weights is None
    (v64, _), (v32, _) = compose(oracle, xyz, rgb, img, t_gt, ypr_gt, np.float64), compose(oracle, xyz, rgb, img, t_gt, ypr_gt, np.float32)
    gap = float(np.abs(v32.astype(np.float64) - v64).max())
    r, wt = res[0].cpu().numpy(), w.cpu().numpy()
    cut = 2.5 * float(scale[0])
    near = (r != -1) & (np.abs(r.astype(np.float64) - cut) <= 3 * gap)
    parity("points within 3 gaps of the threshold", int(near.sum()), 1e-3 * n)
    moved = hit & (np.linalg.norm(rgb - rgb0, axis=1) > 0.5) & ~near
    untouched = ~hit & (r != -1) & ~near
    dropped, kept_out = float((wt[moved] == 0).mean()), float((wt[untouched] == 0).mean())
    print("recoloured by more than 0.5: %d points, %.4f dropped; untouched unmasked: %d points, %.4f dropped; gap %.2e, %d near the cut"
          % (int(moved.sum()), dropped, int(untouched.sum()), kept_out, gap, int(near.sum())))
    assert moved.sum() > 1000 and untouched.sum() > 30000
    assert dropped >= 0.95 and kept_out <= 0.10
    # usable as weights= wherever weights are taken
    out = ops.sampling_loss(ops.Cloud(x, c, order=cloud.order, weights=w), po.packed_pano(im, n_points=n), T(t_gt.reshape(1, 3)), T(ypr_gt.reshape(1, 3)))
    assert float(out[0, 1]) == float(wt[r != -1].sum())


def test_the_robust_chain(ops, oracle):
    """S2, 6 candidates, num_iter 12, robust_iters [4, 8]"""
    from piccolo_amd import omniloc as po
    xyz, rgb, img = scene(oracle, "S2")[:3]
    trans, rot = poses(oracle, "S2", 6)
    n = xyz.shape[0]
    x, c, im = T(xyz), T(rgb), T(img)
    cloud, pano, box = po.packed_cloud(x, c), po.packed_pano(im, n_points=n), po.quantile_box_of(x, 0.05)

    def engine(**kw):
        return ops.GradientDescent(cloud, pano, T(trans), T(rot), box, **kw)
    plain = engine().run(12, history=True)
    gd = engine()
    hist = gd.run_robust(12, [4, 8], "trunc", 2.5, history=True)
    assert hist.shape == (12, 6)
    assert same_bits(hist[:4], plain[:4]) and not same_bits(hist[4:], plain[4:])
    assert gd.cloud is cloud and cloud.weights is None and (gd._robust["plane"][:n] == 0).any()
    # the manual composition through ops: run 4, winner, residuals, weights, weighted_view, run 4 weighted, and again
    man = engine()
    parts = [man.run(4, history=True)]
    for _ in range(2):
        win = man.winner(1)
        row = ops.point_residuals(cloud, pano, win[:, 0:3], win[:, 13:16], packed=True)[0]
        plane, _ = ops.robust_weights(cloud, row, "trunc", 2.5)
        man.cloud = cloud.weighted_view(plane)
        assert man.cloud.data is cloud.data and man.cloud.order is cloud.order and cloud.weights is None
        parts.append(man.run(4, history=True))
    assert same_bits(torch.cat(parts), hist) and same_bits(man.result(), gd.result()) and same_bits(man.winner(1), gd.winner(1))
    # eager == graph replay (twice: the second replays every captured segment), fused == two launches per iteration
    g = engine()
    for _ in range(2):
        g.reset(T(trans), T(rot))
        assert g.run_robust(12, [4, 8], "trunc", 2.5, graph=True) is None
        assert same_bits(g.result(), gd.result())
    assert len(g._graphs) == 2                              # 4 iterations unweighted, 4 iterations over the engine's plane
    two = engine(fuse=False)
    assert same_bits(two.run_robust(12, [4, 8], "trunc", 2.5, history=True), hist) and same_bits(two.result(), gd.result())
    hub = engine()
    hh = hub.run_robust(12, [4, 8], "huber", 1.5, history=True)
    assert same_bits(hh[:4], plain[:4]) and not same_bits(hh[4:], hist[4:])
    # the surface: a plain omniloc_batch returns the same bits before and after a robust one (cloud and engine stayed unweighted)
    base = dict(num_iter=12, num_input=6, lr=0.1, patience=5, factor=0.9)

    def batch(**kw):
        t, r = T(trans).clone(), T(rot).clone()
        out = po.omniloc_batch(im, x, c, t, r, Cfg(**base, **kw), {})
        return [o.clone() for o in out] + [t.cpu(), r.cpu()]
    before = batch()
    rob = batch(robust_iters=[4, 8])
    eager = batch(robust_iters=[4, 8], gd_graph=False)
    after = batch()
    assert all(same_bits(a, b) for a, b in zip(before, after))
    assert all(same_bits(a, b) for a, b in zip(rob, eager))
    win = gd.winner(1)[0].cpu()
    assert same_bits(rob[0].reshape(3), win[0:3]) and same_bits(rob[1].reshape(9), win[3:12]) and same_bits(rob[2].reshape(1), win[12:13])
    assert rob[0].shape == (3, 1) and rob[1].shape == (3, 3) and rob[2].shape == ()
    assert not same_bits(rob[0], before[0])
    assert po.packed_cloud(x, c).weights is None
    from piccolo_amd import localize
    t, r = T(trans).clone(), T(rot).clone()
    ref = localize.refine_image(im, x, c, t, r, Cfg(parallel=True, robust_iters=[4, 8], **base))
    assert all(same_bits(a, b) for a, b in zip(ref, rob[:3]))
