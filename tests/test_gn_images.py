"""GPU tests of the pose information and the Levenberg-Marquardt polish for all images of a shared chain: pcl_pose_information_images,
pcl_gn_refine_images, the ops and omniloc wrappers, omniloc_batch_images_polished and the harness key polish_images_per_launch.
Build-defined: the reference has none of them.  Every assertion but one is BIT equality against the single-image path that
test_pose_information.py and test_gn_refine.py pin to the float64 models; the one number that is not the single call's — the loss of a
polished entry, S1 / M of the polish's own record — is compared bit for bit with that record.

Shapes, scenes and colours are test_robust_images.py's: A = 1025 points on 32 x 64, 3 images (two full 512-slot steps and a one-point
tail); B = 50,001 points on 64 x 128, 2 images (several chunks); images rendered at different poses, 20 % of the colours replaced, per
image for the colour sets."""
import csv
import ctypes

import numpy as np
import pytest
import torch

from conftest import Cfg
from parity_helpers import T
from test_robust_images import FMTS, _write_tree, all_starts, clouds, engines, same_bits, scene

pytestmark = pytest.mark.gpu

WEIGHTS = ("none", "one", "per")
GN_FIELDS = ("trans", "rot", "sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats", "cov")


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def planes_of(ops, n, I, seed=0):
    """(I, pcl_cloud_stride(n)) packed weight planes, multiples of 2^-10 in [0.25, 1] (gn_helpers.weight_plane's kind), another per image,
    0 in the padding"""
    stride = ops._lib.load().pcl_cloud_stride(n)
    out = np.zeros((I, stride), np.float32)
    for i in range(I):
        out[i, :n] = np.floor((0.25 + 0.75 * np.random.default_rng(1000 * seed + n + i).random(n)) * 1024) / 1024
    return T(out)


def poses_of(s, k=1, nan_row=None):
    """one start per image (candidate k of each), optionally with a translation that is not finite in row `nan_row`"""
    trans = np.stack([tr[k] for tr, _ in s["starts"]]).astype(np.float32)
    rot = np.stack([ro[k] for _, ro in s["starts"]]).astype(np.float32)
    if nan_row is not None:
        trans[nan_row, 1] = np.nan
    return T(trans), T(rot)


def winners_of(trans, rot):
    win = torch.full((trans.shape[0], 16), float("nan"), device="cuda")
    win[:, 0:3], win[:, 13:16] = trans, rot
    return win


def setup(ops, oracle, name, fmt, colours, weights):
    """-> (the chain's cloud, per image the cloud its single call takes under its plane, panos, `planes` for the images call, the raw
    (weights tensor, weight_sets) of the C call)"""
    s = scene(oracle, name)
    cloud, singles = clouds(ops, oracle, name, colours)
    panos = [ops.Pano(T(im), fmt=fmt) for im in s["imgs"]]
    I = len(panos)
    if weights == "none":
        return cloud, singles, panos, None, (None, 0)
    pl = planes_of(ops, cloud.n, I)
    if weights == "per":
        return cloud, [c.weighted_view(pl[i]) for i, c in enumerate(singles)], panos, pl, (pl, I)
    # one plane for every image: the cloud's own (a cloud of colour sets carries none: that form goes through the C call, weight_sets = 1)
    if colours == "shared":
        cloud = cloud.weighted_view(pl[0])
    return cloud, [c.weighted_view(pl[0]) for c in singles], panos, None, (pl[0], 1)


def raw_information(ops, cloud, panos, trans, rot, w, wsets):
    lib, I = ops._lib.load(), len(panos)
    info, cov = torch.empty(I, 48, device="cuda"), torch.empty(I, 6, 6, device="cuda")
    nws = lib.pcl_pose_information_workspace_bytes(cloud.n, I)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_uint64 * I)(*[p.data.data_ptr() for p in panos])
    ops._lib.check(lib.pcl_pose_information_images(ops._ptr(cloud.data), ops._ptr(w), wsets, cloud.n, int(cloud.color_sets), arr, I, panos[0].fmt,
                                                   panos[0].H, panos[0].W, ops._ptr(trans), ops._ptr(rot), 3, ops._ptr(info), ops._ptr(cov), ops._ptr(ws),
                                                   nws, ops._stream()), "pcl_pose_information_images")
    return info[:, :36].reshape(I, 6, 6), info[:, 36:42], info[:, 42:47], cov


# ------------------------------------------------------------------------------------------------ 1. the information rows

@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_information_rows_are_the_single_calls(ops, oracle, name, fmt, colours, weights):
    """row i of (H, b, stats, cov) == ops.pose_information of pose i against panorama i, colour set i and plane i alone; pose strides 3
    and 16; rows 0 and 1 differ"""
    s = scene(oracle, name)
    cloud, singles, panos, planes, (w, wsets) = setup(ops, oracle, name, fmt, colours, weights)
    I = len(panos)
    trans, rot = poses_of(s)
    if weights == "one" and colours == "sets":
        rows = raw_information(ops, cloud, panos, trans, rot, w, wsets)
    else:
        rows = ops.pose_information_images(cloud, panos, trans, rot, planes=planes)
        rows16 = ops.pose_information_images_at_winners(cloud, panos, winners_of(trans, rot), planes=planes)
        assert all(same_bits(a, b) for a, b in zip(rows, rows16))
    assert rows[0].shape == (I, 6, 6) and rows[1].shape == (I, 6) and rows[2].shape == (I, 5) and rows[3].shape == (I, 6, 6)
    for i in range(I):
        alone = ops.pose_information(singles[i], panos[i], trans[i:i + 1], rot[i:i + 1])
        for got, want, what in zip(rows, alone, ("H", "b", "stats", "cov")):
            assert same_bits(got[i:i + 1], want), (name, fmt, colours, weights, i, what)
    assert (rows[2][:, 4] == 0).all() and torch.isfinite(rows[3]).all()
    assert not same_bits(rows[0][0], rows[0][1]) and not same_bits(rows[3][0], rows[3][1])
    if weights == "per":                                      # plane 0 for every image is another answer
        wrong = ops.pose_information_images(cloud, panos, trans, rot, planes=planes[:1].expand(I, -1).contiguous())
        assert same_bits(wrong[0][0], rows[0][0]) and not same_bits(wrong[0][1], rows[0][1])


# ------------------------------------------------------------------------------------------------ 2. the polish

@pytest.mark.parametrize("weights", ["none", "per"])
@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_polish_rows_are_the_single_calls(ops, oracle, name, fmt, colours, weights):
    """iters = 4 with the trace: every field and the trace of row i == the single call's; the batch holds a pose that is not finite (status
    1, frozen at k = 0: its blocks return before their point loop) and a pose that runs all iterations — the gate of one moves no other
    pose's bits"""
    s = scene(oracle, name)
    cloud, singles, panos, planes, _ = setup(ops, oracle, name, fmt, colours, weights)
    I = len(panos)
    trans, rot = poses_of(s, nan_row=1)
    res = ops.gauss_newton_refine_images(cloud, panos, trans, rot, iters=4, trace=True, planes=planes)
    res16 = ops.gauss_newton_refine_images_at_winners(cloud, panos, winners_of(trans, rot), iters=4, trace=True, planes=planes)
    assert res["trace"].shape == (5, I, 16)
    for i in range(I):
        alone = ops.gauss_newton_refine(singles[i], panos[i], trans[i:i + 1], rot[i:i + 1], iters=4, trace=True)
        for key in GN_FIELDS:
            assert same_bits(res[key][i:i + 1], alone[key]), (name, fmt, colours, weights, i, key)
            assert same_bits(res16[key][i:i + 1], alone[key]), (name, fmt, colours, weights, i, key)
        assert same_bits(res["trace"][:, i:i + 1], alone["trace"]) and same_bits(res16["trace"][:, i:i + 1], alone["trace"])
    status, evals = res["status"].tolist(), res["evaluations"].tolist()
    assert status[1] == 1 and evals[1] == 1 and (res["trace"][1:, 1] == 0).all() and torch.isnan(res["cov"][1]).all()
    assert status[0] == 0 and evals[0] == 5 and float(res["accepted"][0]) > 1 and float(res["sigma2"][0]) < float(res["sigma2_start"][0])
    # the same batch without the frozen pose: row 0 keeps its bits
    trans2, rot2 = poses_of(s)
    res2 = ops.gauss_newton_refine_images(cloud, panos, trans2, rot2, iters=4, trace=True, planes=planes)
    assert all(same_bits(res[key][0], res2[key][0]) for key in GN_FIELDS) and float(res2["status"][1]) != 1


# ------------------------------------------------------------------------------------------------ 3. more images than one launch names

def test_seventy_images_run_in_two_groups(ops, oracle):
    """70 poses / panoramas / colour sets / planes at iters = 1: the pass runs once per 64 addresses, the colour set, the plane and the
    partial row counted from the call's first image; rows 0 and 62 .. 69 == their single calls"""
    s = scene(oracle, "A")
    x = T(s["xyz"])
    rng = np.random.default_rng(3)
    rgbs = [T(np.roll(s["rgb"], k, axis=0)) for k in range(70)]
    keep = [0] + list(range(62, 70))
    singles = {i: ops.Cloud(x, rgbs[i]) for i in keep}
    cloud = ops.Cloud.with_color_sets(x, rgbs, order=singles[0].order)
    p = [ops.Pano(T(im), fmt="u8") for im in s["imgs"]]
    panos = [p[k % 3] for k in range(70)]
    tr, ro = s["starts"][0]
    trans = T(np.stack([tr[k % 4] + 0.01 * rng.random(3).astype(np.float32) for k in range(70)]))
    rot = T(np.stack([ro[k % 4] for k in range(70)]))
    planes = planes_of(ops, cloud.n, 70, seed=7)
    res = ops.gauss_newton_refine_images(cloud, panos, trans, rot, iters=1, trace=True, planes=planes)
    info = ops.pose_information_images(cloud, panos, trans, rot, planes=planes)
    assert res["trace"].shape == (2, 70, 16)
    for i in keep:
        single = singles[i].weighted_view(planes[i])
        alone = ops.gauss_newton_refine(single, panos[i], trans[i:i + 1], rot[i:i + 1], iters=1, trace=True)
        for key in GN_FIELDS:
            assert same_bits(res[key][i:i + 1], alone[key]), (i, key)
        assert same_bits(res["trace"][:, i:i + 1], alone["trace"]), i
        for got, want in zip(info, ops.pose_information(single, panos[i], trans[i:i + 1], rot[i:i + 1])):
            assert same_bits(got[i:i + 1], want), i
    assert not same_bits(res["H"][0], res["H"][64]) and not same_bits(res["H"][64], res["H"][65])


# ------------------------------------------------------------------------------------------------ 4. at the winners of the chains

@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_polish_at_the_winners_of_the_chains(ops, oracle, name, colours):
    """the images chain and the robust weight-set chain (test_robust_images.engines: A 3 x 4 candidates, B 2 x 6), run; then ONE polish of
    all winners — under the robust chain's planes — row i == gauss_newton_refine_at_winners of image i's single cloud under that plane"""
    from piccolo_amd import omniloc as po
    fmt = "f16" if name == "B" else "u8"
    s = scene(oracle, name)
    multi, _, I, per = engines(ops, oracle, name, colours, fmt)
    cloud, singles = clouds(ops, oracle, name, colours)
    panos = multi._panos
    # the robust weight-set chain
    multi.run_robust(12, [4, 8], "trunc", 2.5)
    wins, planes = multi.winners(I), multi.weight_planes()
    assert not same_bits(planes[0], planes[1])
    res = ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=4, planes=planes)
    cov = ops.pose_information_images_at_winners(cloud, panos, wins, planes=planes)[3]
    for i in range(I):
        single = singles[i].weighted_view(planes[i])
        alone = ops.gauss_newton_refine_at_winners(single, panos[i], wins[i:i + 1].contiguous(), iters=4)
        for key in GN_FIELDS:
            assert same_bits(res[key][i:i + 1], alone[key]), (name, colours, i, key)
        assert same_bits(cov[i:i + 1], ops.pose_information_at_winners(single, panos[i], wins[i:i + 1].contiguous())[3])
    # the plain images chain
    tr, ro = all_starts(s)
    plain = ops.GradientDescent(cloud, panos[0], tr, ro, po.quantile_box_of(T(s["xyz"]), 0.05))
    plain.set_pano_groups(panos)
    plain.run(12)
    wins = plain.winners(I)
    res = ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=4)
    for i in range(I):
        alone = ops.gauss_newton_refine_at_winners(singles[i], panos[i], wins[i:i + 1].contiguous(), iters=4)
        for key in GN_FIELDS:
            assert same_bits(res[key][i:i + 1], alone[key]), (name, colours, i, key)


# ------------------------------------------------------------------------------------------------ 5. the surface

BASE = dict(num_iter=12, num_input=6, lr=0.1, patience=5, factor=0.9)
CHAINS = {"plain": {}, "robust": dict(robust_iters=[4, 8]), "prune": dict(prune_iters=4, prune_keep=3)}


def expected_losses(ops, po, ims, x, rgb, starts, cfg):
    """(took, loss) per image from the pieces: the chain as the entry point runs it, then item 4's call at its winners — float32(S1) /
    float32(M) of that record where the polish took a step, else the chain's own loss"""
    I = len(ims)
    panos = po._chain_panos(ims, x.shape[0])
    robust = po.robust_schedule(cfg)
    tr, ro = torch.cat([t.clone() for t in starts[0]]), torch.cat([r.clone() for r in starts[1]])
    gd = po._refine(x, rgb, panos, tr, ro, po.quantile_box_of(x, 0.05), cfg, True, weight_sets=I if robust is not None else 0)
    wins = gd.winners(I)
    planes = gd.weight_planes() if robust is not None else None
    cloud = po.packed_cloud_sets(x, rgb) if isinstance(rgb, list) else po.packed_cloud(x, rgb)
    gn = po.gn_schedule(cfg)
    res = ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=gn[0], planes=planes, **gn[1])
    acc, status, stats, chain = res["accepted"].cpu().numpy(), res["status"].cpu().numpy(), res["stats"].cpu().numpy(), wins[:, 12].cpu().numpy()
    took = (acc > 1) & ((status == 0) | (status == 3))
    return took, [np.float32(stats[i, 1]) / np.float32(stats[i, 0]) if took[i] else chain[i] for i in range(I)]


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_the_surface(ops, oracle, colours, chain):
    """omniloc_batch_images_polished entry i against omniloc_batch(imgs[i], xyz, rgb_i, ...) under the same cfg: t, R and cov bit for bit;
    the loss == float32(S1) / float32(M) of the polish's record where it took a step, the chain's own where it did not; with
    pose_covariance alone the first three entries are the chain's.  Both branches occur."""
    from piccolo_amd import omniloc as po
    s = scene(oracle, "B")
    n = s["xyz"].shape[0]
    x, ims = T(s["xyz"]), [T(im) for im in s["imgs"]]
    I = len(ims)
    rgbs = [T(s["rgb"])] * I if colours == "shared" else [T(r) for r in s["rgbs"]]
    rgb = rgbs[0] if colours == "shared" else rgbs
    if colours == "shared" and chain != "robust":
        # (a plain chain of shared colours cuts the cloud by the plan of all its candidates: the bits are the single call's where the
        # two plans agree, omniloc_batch_images' own caveat — they do at this shape)
        lib, a, b = ops._lib.load(), [ctypes.c_int(), ctypes.c_int()], [ctypes.c_int(), ctypes.c_int()]
        for per in (6, 3) if chain == "prune" else (6,):
            assert lib.pcl_gd_plan(n, per, ctypes.byref(a[0]), ctypes.byref(a[1]), None) == 0
            assert lib.pcl_gd_plan(n, I * per, ctypes.byref(b[0]), ctypes.byref(b[1]), None) == 0
            assert a[0].value == b[0].value, (per, a[0].value, b[0].value)

    def starts():
        return [T(tr).clone() for tr, _ in s["starts"]], [T(ro).clone() for _, ro in s["starts"]]

    def images(fn, **kw):
        tl, rl = starts()
        out = fn(ims, x, rgb, tl, rl, Cfg(**BASE, **CHAINS[chain], **kw))
        return out, [t.cpu() for t in tl], [r.cpu() for r in rl]

    def singles(**kw):
        tl, rl = starts()
        out = [po.omniloc_batch(ims[i], x, rgbs[i], tl[i], rl[i], Cfg(**BASE, **CHAINS[chain], **kw), {}) for i in range(I)]
        return out, [t.cpu() for t in tl], [r.cpu() for r in rl]
    alone_fn = po.omniloc_batch_images_robust if chain == "robust" else po.omniloc_batch_images
    base, base_t, base_r = images(alone_fn)
    seen = set()
    for kw in (dict(gn_iters=3), dict(gn_iters=3, pose_covariance=True), dict(gn_iters=1, gn_step_cap=1e-30, pose_covariance=True)):
        got, got_t, got_r = images(po.omniloc_batch_images_polished, **kw)
        one, one_t, one_r = singles(**kw)
        took, losses = expected_losses(ops, po, ims, x, rgb, starts(), Cfg(**BASE, **CHAINS[chain], **kw))
        for i in range(I):
            assert len(got[i]) == len(one[i]) == (4 if "pose_covariance" in kw else 3)
            assert same_bits(got[i][0], one[i][0]) and same_bits(got[i][1], one[i][1]), (colours, chain, kw, i)
            assert got[i][0].shape == (3, 1) and got[i][1].shape == (3, 3) and got[i][2].shape == ()
            if "pose_covariance" in kw:
                assert got[i][3].shape == (6, 6) and same_bits(got[i][3], one[i][3]), (colours, chain, kw, i)
            assert np.float32(got[i][2].item()).tobytes() == np.float32(losses[i]).tobytes(), (colours, chain, kw, i, got[i][2], losses[i])
            if took[i]:
                # the single call's loss is the forward launch's sum of the same terms in another order: each within n 2^-24 of the exact one
                assert abs(float(got[i][2]) - float(one[i][2])) <= 2 * n * 2.0 ** -24 * abs(float(one[i][2]))
                assert not same_bits(got[i][0], base[i][0])
            else:
                assert all(same_bits(a, b) for a, b in zip(got[i][:3], base[i])) and same_bits(got[i][2], one[i][2])
            seen.add(bool(took[i]))
            assert same_bits(got_t[i], one_t[i]) and same_bits(got_r[i], one_r[i])             # the written-back leaves stay the chain's
            assert same_bits(got_t[i], base_t[i]) and same_bits(got_r[i], base_r[i])
    assert seen == {True, False}
    # pose_covariance alone: the chain's three entries, and the single call's covariance
    got = images(po.omniloc_batch_images_polished, pose_covariance=True)[0]
    one = singles(pose_covariance=True)[0]
    for i in range(I):
        assert len(got[i]) == 4 and all(same_bits(a, b) for a, b in zip(got[i][:3], base[i]))
        assert same_bits(got[i][3], one[i][3]) and torch.isfinite(got[i][3]).all()
    assert not same_bits(got[0][3], got[1][3])
    # one image forwards to omniloc_batch
    tl, rl = starts()
    first = po.omniloc_batch_images_polished(ims[:1], x, rgbs[0], tl[:1], rl[:1], Cfg(**BASE, **CHAINS[chain], gn_iters=3, pose_covariance=True))
    ref = singles(gn_iters=3, pose_covariance=True)[0][0]
    assert len(first) == 1 and all(same_bits(a, b) for a, b in zip(first[0], ref))


# ------------------------------------------------------------------------------------------------ 6. the harness

HARNESS = dict(num_trans=12, xy_only=False, yaw_only=False, num_yaw=4, num_pitch=2, num_roll=2, criterion="loss_histogram", num_intermediate=8,
               num_input=4, num_split_h=4, num_split_w=4, lr=0.1, num_iter=12, patience=5, factor=0.8, out_of_room_quantile=0.05, sample_rate=1,
               parallel=True, num_bins=256, gn_iters=3, pose_covariance=True)


@pytest.mark.parametrize("sharpen", [True, False])
def test_harness_groups_give_the_one_at_a_time_rows(tmp_path, sharpen):
    """polish_images_per_launch = 3 (one group of the three frames) and = 1 write the same CSV rows in every pose column, and the same
    finite sigma_t / sigma_r; per-image colour sets (sharpen_color) and shared colours"""
    from piccolo_amd import localize
    from test_dataset_harness import _csv_without_time
    root = tmp_path / "stanford"
    _write_tree(root)
    rows = {}
    for group in (1, 3):
        log = tmp_path / ("log%d" % group)
        cfg = Cfg(dataset="Stanford2D-3D-S", area=3, sharpen_color=sharpen, images_per_launch=1, polish_images_per_launch=group, **HARNESS)
        table = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
        assert table.shape == (3, 16) and not np.isnan(table).any()
        rows[group] = (_csv_without_time(log / "stanford_results.csv"), table)
    assert rows[1][0] == rows[3][0] and len(rows[1][0]) == 4
    assert np.array_equal(rows[1][1][:, :12], rows[3][1][:, :12]) and np.array_equal(rows[1][1][:, 13:15], rows[3][1][:, 13:15])
    with open(tmp_path / "log3" / "stanford_results.csv") as f:
        full = list(csv.reader(f))
    assert full[0][-2:] == ["sigma_t (m)", "sigma_r (degrees)"] and full[0][:-2] == localize.STANFORD_HEADER
    for r in full[1:]:
        assert len(r) == len(full[0]) and all(np.isfinite(float(v)) and float(v) > 0 for v in r[-2:])
