"""GPU tests of the robust chain over several query images of one cloud: pcl_point_residuals_images, pcl_robust_weights_rows, the weight-set
instances of the loss kernel, pcl_gd_run_weight_sets, omniloc_batch_images_robust and the harness key robust_images_per_launch.
Build-defined: the reference has none of them.  Every assertion is BIT equality against the single-image path that test_point_weights.py and
test_point_residuals.py pin to the oracle — no numeric tolerance.

Shapes: A = 1025 points on 32 x 64, 3 images x 4 candidates (two full 512-point steps and a one-point tail; two poses per block, groups
must not straddle images) and 3 x 3 (one pose per block); B = 50,001 points on 64 x 128, 2 images x 6 candidates (several chunks).  The
images are rendered at different ground-truth poses (oracle.make_pano_u8: exact k/255 texels) and the cloud's colours are replaced by
uniform random ones on 20 % of the points after the render — per image on another 20 % for the per-image colour sets."""
import csv
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import Cfg
from parity_helpers import T

pytestmark = pytest.mark.gpu

FMTS = ("f16", "u8", "f32")
SHAPES = {"A": (1025, 32, 64, 3, 4), "A3": (1025, 32, 64, 3, 3), "B": (50001, 64, 128, 2, 6)}
KINDS = [("trunc", 2.5), ("huber", 1.5)]


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


_SCENES = {}


def scene(oracle, name):
    """of a shape, computed once and shared: xyz, the shared recoloured rgb, one recoloured rgb per image, the images, per image the
    starting poses (trans, rot)"""
    if name not in _SCENES:
        from piccolo_amd import synth
        n, H, W, I, per = SHAPES[name]
        xyz, rgb0 = synth.box_room(n, seed=n % 89)
        imgs, starts = [], []
        for i in range(I):
            t_gt, ypr_gt = synth.gt_pose(n % 97 + 7 * i)
            imgs.append(oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb0, (H, W)).astype(np.float32) / 255)
            starts.append(synth.start_poses(np.asarray(t_gt, np.float32), np.asarray(ypr_gt, np.float32), per, seed=n + i))

        def recolour(seed):
            rng = np.random.default_rng(seed)
            hit = rng.random(n) < 0.2
            rgb = rgb0.copy()
            rgb[hit] = rng.random((int(hit.sum()), 3)).astype(np.float32)
            return rgb
        _SCENES[name] = dict(xyz=xyz, rgb=recolour(5), rgbs=[recolour(11 + i) for i in range(I)], imgs=imgs, starts=starts)
    return _SCENES[name]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def clouds(ops, oracle, name, colours):
    """-> (the chain's cloud, per image the cloud its single-image call takes): "shared" colours or per-image colour "sets" """
    s = scene(oracle, name)
    x = T(s["xyz"])
    if colours == "shared":
        c = ops.Cloud(x, T(s["rgb"]))
        return c, [c] * len(s["imgs"])
    singles = [ops.Cloud(x, T(r)) for r in s["rgbs"]]
    return ops.Cloud.with_color_sets(x, [T(r) for r in s["rgbs"]], order=singles[0].order), singles


def all_starts(s):
    return T(np.concatenate([tr for tr, _ in s["starts"]])), T(np.concatenate([ro for _, ro in s["starts"]]))


# ------------------------------------------------------------------------------------------------ the stand-alone calls

@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_residual_rows_are_the_single_calls_rows(ops, oracle, name, fmt, colours):
    """row i == ops.point_residuals of pose i against panorama i (and colour set i) alone: caller and packed order, pose strides 3 and 16"""
    s = scene(oracle, name)
    cloud, singles = clouds(ops, oracle, name, colours)
    panos = [ops.Pano(T(im), fmt=fmt) for im in s["imgs"]]
    I = len(panos)
    trans = T(np.stack([tr[1] for tr, _ in s["starts"]]))
    rot = T(np.stack([ro[1] for _, ro in s["starts"]]))
    win = torch.full((I, 16), float("nan"), device="cuda")
    win[:, 0:3], win[:, 13:16] = trans, rot
    for packed in (False, True):
        rows = ops.point_residuals_images(cloud, panos, trans, rot, packed=packed)
        rows16 = ops.point_residuals_images_at_winners(cloud, panos, win, packed=packed)
        assert rows.shape == (I, cloud.n) and same_bits(rows, rows16)
        for i in range(I):
            alone = ops.point_residuals(singles[i], panos[i], trans[i:i + 1], rot[i:i + 1], packed=packed)
            assert same_bits(rows[i:i + 1], alone), (name, fmt, colours, packed, i)
        assert (rows >= 0).any() and (rows == -1).any()
        assert not same_bits(rows[0], rows[1])                    # (another panorama and pose: a kernel that reads image 0 for all would fail above)
    # in place into a buffer of the caller
    out = torch.empty(I, cloud.n, device="cuda")
    assert ops.point_residuals_images_at_winners(cloud, panos, win, packed=True, out=out) is out and same_bits(out, rows)


def test_residual_rows_of_more_images_than_one_launch_names(ops, oracle):
    """70 poses / panoramas: two launches (64 addresses travel per launch), the colour set counted from the call's first image"""
    s = scene(oracle, "A")
    x = T(s["xyz"])
    rng = np.random.default_rng(3)
    rgbs = [T(np.roll(s["rgb"], k, axis=0)) for k in range(70)]
    singles = [ops.Cloud(x, r) for r in rgbs[:1] + rgbs[62:]]
    cloud = ops.Cloud.with_color_sets(x, rgbs, order=singles[0].order)
    p = [ops.Pano(T(im), fmt="u8") for im in s["imgs"]]
    panos = [p[k % 3] for k in range(70)]
    tr, ro = s["starts"][0]
    trans = T(np.stack([tr[k % 4] + 0.01 * rng.random(3).astype(np.float32) for k in range(70)]))
    rot = T(np.stack([ro[k % 4] for k in range(70)]))
    rows = ops.point_residuals_images(cloud, panos, trans, rot, packed=True)
    for j, i in enumerate([0] + list(range(62, 70))):
        assert same_bits(rows[i:i + 1], ops.point_residuals(singles[j], panos[i], trans[i:i + 1], rot[i:i + 1], packed=True)), i


@pytest.mark.parametrize("kind,k", KINDS)
def test_weight_rows_are_the_single_calls_planes(ops, oracle, kind, k):
    """plane i, scale i == ops.robust_plane of row i alone; among the rows one with M = 0 (all masked), one holding NaNs and one all NaN"""
    s = scene(oracle, "B")
    cloud, _ = clouds(ops, oracle, "B", "shared")
    panos = [ops.Pano(T(im), fmt="f16") for im in s["imgs"]]
    n = cloud.n
    rows = ops.point_residuals_images(cloud, panos, T(np.stack([tr[0] for tr, _ in s["starts"]])), T(np.stack([ro[0] for _, ro in s["starts"]])),
                                      packed=True)
    masked = torch.full((1, n), -1.0, device="cuda")
    holed = rows[:1].clone()
    holed[0, ::7] = float("nan")
    holed[0, 5::11] = float("inf")
    rows = torch.cat([rows, masked, holed, torch.full((1, n), float("nan"), device="cuda"),
                      torch.where(rows[1:2] == -1, rows[1:2], rows[1:2] * 0.5)]).contiguous()
    R = rows.shape[0]
    planes, scales = ops.robust_planes(n, rows, kind, k)
    stride = ops._lib.load().pcl_cloud_stride(n)
    assert planes.shape == (R, stride) and scales.shape == (R, 2) and not torch.isnan(planes).any()
    for i in range(R):
        plane, scale = ops.robust_plane(n, rows[i].clone(), kind, k)
        assert same_bits(planes[i], plane), (kind, i)
        assert same_bits(scales[i], scale), (kind, i, scales[i], scale)
    assert (planes[2, :n] == 1).all() and scales[2].tolist() == [0.0, 0.0]               # M = 0: the unit plane
    assert (planes[3, :n][torch.isnan(rows[3]) | torch.isinf(rows[3])] == 0).all() and float(scales[3, 0]) > 0
    assert (planes[4] == 0).all() and torch.isnan(scales[4, 0]) and float(scales[4, 1]) == n
    assert (planes[:, n:] == 0).all() and not same_bits(planes[0], planes[1])
    # in place, with buffers and a workspace of the caller: the same bits again
    ws = torch.empty(ops._lib.load().pcl_robust_weights_rows_workspace_bytes(n, R), dtype=torch.uint8, device="cuda")
    p2, s2 = ops.robust_planes(n, rows, kind, k, torch.empty_like(planes), torch.empty_like(scales), ws)
    assert same_bits(p2, planes) and same_bits(s2, scales)


# ------------------------------------------------------------------------------------------------ the loss instances

def engines(ops, oracle, name, colours, fmt, **kw):
    """-> (the weight-set engine over all images, per image the single-image engine, I, per)"""
    from piccolo_amd import omniloc as po
    s = scene(oracle, name)
    cloud, singles = clouds(ops, oracle, name, colours)
    panos = [ops.Pano(T(im), fmt=fmt) for im in s["imgs"]]
    box = po.quantile_box_of(T(s["xyz"]), 0.05)
    I, per = len(panos), s["starts"][0][0].shape[0]
    tr, ro = all_starts(s)
    multi = ops.GradientDescent(cloud, panos[0], tr, ro, box, weight_sets=I, **kw)
    multi.set_pano_groups(panos)
    alone = [ops.GradientDescent(singles[i], panos[i], T(s["starts"][i][0]), T(s["starts"][i][1]), box, **kw) for i in range(I)]
    return multi, alone, I, per


def restart(gd, tr, ro):
    """new starting poses: reset() clears the pose records' panoramas, so they are named again"""
    gd.reset(tr, ro)
    gd.set_pano_groups(gd._panos)


@pytest.mark.parametrize("fuse", [None, False])
@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["A", "A3"])
def test_weight_set_loss_instances(ops, oracle, name, fmt, colours, fuse):
    """Three iterations (the second and third forwards sit at poses the gradients of the ones before made; the state holds Adam's moments
    of them): with I identical planes of general weights every image's loss history, state and pose equal the one-plane weighted run's,
    with unit planes — and with the planes off — the unweighted single-image run's.  A: two poses per block, A3: one; fused and two-launch
    forms; the three texel formats; shared colours and colour sets."""
    multi, alone, I, per = engines(ops, oracle, name, colours, fmt, fuse=fuse)
    n = multi.cloud.n
    nch, G, fused = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert ops._lib.load().pcl_gd_plan_weight_sets(n, I * per, I, ctypes.byref(multi.hyper), ctypes.byref(nch), ctypes.byref(G), ctypes.byref(fused)) == 0
    assert G.value == (2 if per % 2 == 0 else 1) and fused.value == (0 if fuse is False else 1)
    rng = np.random.default_rng(17)
    w = np.zeros(multi.weight_planes().shape[1], np.float32)
    w[:n] = (rng.random(n) * 2).astype(np.float32)
    w[:n][rng.random(n) < 0.1] = 0
    tr, ro = all_starts(scene(oracle, name))

    def check(hist, make_single):
        res, win = multi.result(), multi.winners(I)
        for i in range(I):
            g = make_single(alone[i])
            g.reset(tr[i * per:(i + 1) * per], ro[i * per:(i + 1) * per])
            h = g.run(3, history=True)
            assert same_bits(hist[:, i * per:(i + 1) * per], h), (name, fmt, colours, fuse, i)
            assert same_bits(res[i * per:(i + 1) * per], g.result()) and same_bits(win[i:i + 1], g.winner(1))
    # the planes off: the plain (or colour-set) instances under the single-image plan
    check(multi.run(3, history=True), lambda g: g)
    plain = multi.result()
    # unit planes
    restart(multi, tr, ro)
    multi.weight_planes().copy_(T((np.arange(w.size) < n).astype(np.float32)).expand(I, -1))
    multi.weight_planes_on()
    check(multi.run(3, history=True), lambda g: g)
    assert same_bits(multi.result(), plain)
    # I identical planes of general weights

    def weighted(g):
        g.cloud = g.cloud.weighted_view(T(w))
        return g
    restart(multi, tr, ro)
    multi.weight_planes().copy_(T(w).expand(I, -1))
    hist = multi.run(3, history=True)
    check(hist, weighted)
    assert not same_bits(multi.result(), plain)
    # another plane for the LAST image only: the other images' bits stay, that image's move
    restart(multi, tr, ro)
    multi.weight_planes()[I - 1].mul_(0.5)
    multi.weight_planes()[I - 1, :n:3] = 0
    other = multi.run(3, history=True)
    assert same_bits(other[:, :(I - 1) * per], hist[:, :(I - 1) * per]) and not same_bits(other[:, (I - 1) * per:], hist[:, (I - 1) * per:])


# ------------------------------------------------------------------------------------------------ the chain

@pytest.mark.parametrize("kind,k", KINDS)
@pytest.mark.parametrize("colours", ["shared", "sets"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_chain_is_every_images_own_robust_chain(ops, oracle, name, colours, kind, k):
    """num_iter 12, robust_iters [4, 8]: the loss history's columns of image i == the single-image run_robust history of image i, fused and
    fuse=False; eager == graph replay, replayed twice; the I planes differ from one another after the first re-weighting"""
    fmt = "f16" if name == "B" else "u8"
    multi, alone, I, per = engines(ops, oracle, name, colours, fmt)
    n = multi.cloud.n
    hist = multi.run_robust(12, [4, 8], kind, k, history=True)
    assert hist.shape == (12, I * per)
    singles = [g.run_robust(12, [4, 8], kind, k, history=True) for g in alone]
    for i in range(I):
        assert same_bits(hist[:, i * per:(i + 1) * per], singles[i]), (name, colours, kind, i)
        assert same_bits(multi.result()[i * per:(i + 1) * per], alone[i].result())
        assert same_bits(multi.weight_planes()[i], alone[i]._robust["plane"])
        assert same_bits(multi._robust["scale"].view(I, 2)[i], alone[i]._robust["scale"])
    assert same_bits(multi.winners(I), torch.cat([g.winner(1) for g in alone]))
    assert multi.cloud.weights is None
    final = multi.result()
    # the planes after the FIRST re-weighting differ from image to image (a kernel that read plane 0 for every image would pass otherwise)
    tr, ro = all_starts(scene(oracle, name))
    restart(multi, tr, ro)
    multi.robust_clear()
    first = multi.run(4, history=True)
    assert same_bits(first, hist[:4])
    planes, scales = multi.robust_reweight(kind, k)
    assert planes.shape == (I, planes.shape[1]) and (planes[:, :n] < 1).any(1).all()
    for i in range(I):
        for j in range(i + 1, I):
            assert not same_bits(planes[i], planes[j]), (i, j)
    assert same_bits(multi.run(4, history=True), hist[4:8])
    # the two-launch form
    two = engines(ops, oracle, name, colours, fmt, fuse=False)[0]
    assert same_bits(two.run_robust(12, [4, 8], kind, k, history=True), hist) and same_bits(two.result(), final)
    # eager == graph replay, twice (the second replays every captured segment)
    g = engines(ops, oracle, name, colours, fmt)[0]
    for _ in range(2):
        restart(g, tr, ro)
        assert g.run_robust(12, [4, 8], kind, k, graph=True) is None
        assert same_bits(g.result(), final)
    assert len(g._graphs) == 2                              # 4 iterations unweighted, 4 iterations over the engine's planes


def test_engine_refusals(ops, oracle):
    from piccolo_amd import omniloc as po
    s = scene(oracle, "A")
    cloud, _ = clouds(ops, oracle, "A", "shared")
    pano = ops.Pano(T(s["imgs"][0]), fmt="u8")
    box = po.quantile_box_of(T(s["xyz"]), 0.05)
    tr, ro = all_starts(s)
    with pytest.raises(ValueError, match="weight_sets"):
        ops.GradientDescent(cloud, pano, tr, ro, box, weight_sets=5)                    # 12 candidates do not split into 5 images
    with pytest.raises(ValueError, match="weight_sets"):
        ops.GradientDescent(cloud, pano, tr, ro, box, weight_sets=3, depth_mask=True)
    with pytest.raises(ValueError, match="weight_sets"):
        ops.GradientDescent(clouds(ops, oracle, "A", "sets")[0], pano, tr, ro, box, weight_sets=2)       # 3 colour sets, 2 weight sets
    plain = ops.GradientDescent(cloud, pano, tr, ro, box)
    plain.set_pano_groups([ops.Pano(T(im), fmt="u8") for im in s["imgs"]])
    with pytest.raises(ValueError, match="one image"):
        plain.robust_reweight()
    with pytest.raises(ValueError, match="weight_sets"):
        plain.weight_planes()
    with pytest.raises(ValueError, match="not pruned"):
        ops.GradientDescent(cloud, pano, tr, ro, box, weight_sets=3).pruned(2)


# ------------------------------------------------------------------------------------------------ the surface

@pytest.mark.parametrize("colours", ["shared", "sets"])
def test_the_surface(ops, oracle, colours):
    """omniloc_batch_images_robust entry i == omniloc_batch(imgs[i], xyz, rgb_i, ...) under the same robust cfg: t, R, loss and the leaf rows
    written back; a plain omniloc_batch_images returns the same bits before and after; the cached packed cloud stays unweighted"""
    from piccolo_amd import omniloc as po
    s = scene(oracle, "B")
    x, ims = T(s["xyz"]), [T(im) for im in s["imgs"]]
    rgbs = [T(s["rgb"])] * len(ims) if colours == "shared" else [T(r) for r in s["rgbs"]]
    rgb = rgbs[0] if colours == "shared" else rgbs
    base = dict(num_iter=12, num_input=6, lr=0.1, patience=5, factor=0.9)

    def starts():
        return [T(tr).clone() for tr, _ in s["starts"]], [T(ro).clone() for _, ro in s["starts"]]

    def images(fn, **kw):
        tl, rl = starts()
        out = fn(ims, x, rgb, tl, rl, Cfg(**base, **kw))
        return [[o.clone() for o in e] + [t.cpu(), r.cpu()] for e, t, r in zip(out, tl, rl)]

    def equal(a, b):
        return all(all(same_bits(p, q) for p, q in zip(ea, eb)) for ea, eb in zip(a, b)) and len(a) == len(b)
    before = images(po.omniloc_batch_images)
    rob = images(po.omniloc_batch_images_robust, robust_iters=[4, 8])
    eager = images(po.omniloc_batch_images_robust, robust_iters=[4, 8], gd_graph=False)
    again = images(po.omniloc_batch_images_robust, robust_iters=[4, 8])                 # (the cached engine, reset)
    after = images(po.omniloc_batch_images)
    assert equal(before, after) and equal(rob, eager) and equal(rob, again) and not equal(rob, before)
    tl, rl = starts()
    for i, im in enumerate(ims):
        one = po.omniloc_batch(im, x, rgbs[i], tl[i], rl[i], Cfg(**base, robust_iters=[4, 8]), {})
        assert po.packed_pano(im, n_points=x.shape[0]).fmt == po.packed_pano(ims[0], n_points=x.shape[0]).fmt
        assert all(same_bits(a, b) for a, b in zip(one, rob[i][:3])), i
        assert same_bits(tl[i].cpu(), rob[i][3]) and same_bits(rl[i].cpu(), rob[i][4])
        assert rob[i][0].shape == (3, 1) and rob[i][1].shape == (3, 3) and rob[i][2].shape == ()
    hub = images(po.omniloc_batch_images_robust, robust_iters=[4, 8], robust_kind="huber", robust_k=1.5)
    assert not equal(hub, rob)
    for r in rgbs:
        assert po.packed_cloud(x, r).weights is None
    # one image forwards to omniloc_batch
    tl, rl = starts()
    single = po.omniloc_batch_images_robust(ims[:1], x, rgbs[0], tl[:1], rl[:1], Cfg(**base, robust_iters=[4, 8]))
    assert len(single) == 1 and all(same_bits(a, b) for a, b in zip(single[0], rob[0][:3])) and same_bits(tl[0].cpu(), rob[0][3])


# ------------------------------------------------------------------------------------------------ the harness

HH, HW, HN = 64, 128, 20_000
HARNESS = dict(num_trans=12, xy_only=False, yaw_only=False, num_yaw=4, num_pitch=2, num_roll=2, criterion="loss_histogram", num_intermediate=8,
               num_input=4, num_split_h=4, num_split_w=4, lr=0.1, num_iter=12, patience=5, factor=0.8, out_of_room_quantile=0.05, sample_rate=1,
               parallel=True, num_bins=256, robust_iters=[4, 8])


def _write_tree(root):
    """a Stanford2D-3D-S layout of one small synthetic room with three frames, as tests/test_dataset_harness.py builds it"""
    from PIL import Image
    from piccolo_amd import ops, synth
    from test_dataset_harness import POSES, _euler_for_stanford, _write_cloud
    xyz, rgb = synth.box_room(HN, 21)
    xyz, rgb8 = xyz.astype(np.float32), np.clip(np.round(rgb * 255), 0, 255).astype(np.uint8)
    _write_cloud(str(root / "pcd_not_aligned/area_3/office_1.txt"), xyz, rgb8)
    os.makedirs(root / "pano/area_3")
    os.makedirs(root / "pose/area_3")
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb8.astype(np.float32) / np.float32(255)).cuda()
    for k, (t, ypr) in enumerate(POSES + [(np.array([0.2, 0.3, 0.0], np.float32), np.array([2.0, 0.01, 0.02], np.float32))]):
        pano = ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t), torch.from_numpy(ypr)), C, (HH, HW)).cpu().numpy().astype(np.uint8)
        stem = "camera_c%03d_office_1_frame_equirectangular_domain" % k
        Image.fromarray(pano).save(root / "pano/area_3" / (stem + "_rgb.png"))
        with open(root / "pose/area_3" / (stem + "_pose.json"), "w") as f:
            json.dump({"camera_location": [float(v) for v in t],
                       "final_camera_rotation": _euler_for_stanford(synth.rot_from_ypr_np(ypr).astype(np.float64))}, f)


@pytest.mark.parametrize("sharpen", [True, False])
def test_harness_groups_give_the_one_at_a_time_rows(tmp_path, sharpen):
    """robust_images_per_launch = 2 (a group of two and a single frame) and = 1 write the same CSV rows, per-image colour sets
    (sharpen_color) and shared colours"""
    from piccolo_amd import localize
    from test_dataset_harness import _csv_without_time
    root = tmp_path / "stanford"
    _write_tree(root)
    rows = {}
    for group in (1, 2):
        log = tmp_path / ("log%d" % group)
        cfg = Cfg(dataset="Stanford2D-3D-S", area=3, sharpen_color=sharpen, images_per_launch=1, robust_images_per_launch=group, **HARNESS)
        table = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
        assert table.shape == (3, 16) and not np.isnan(table).any()
        rows[group] = (_csv_without_time(log / "stanford_results.csv"), table)
    assert rows[1][0] == rows[2][0] and len(rows[1][0]) == 4
    assert np.array_equal(rows[1][1][:, :15], rows[2][1][:, :15])
    with open(tmp_path / "log2" / "stanford_results.csv") as f:
        assert len(list(csv.reader(f))) == 4
