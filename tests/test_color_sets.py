"""GPU tests of per-image colour sets: one point set, one colour set per query image, one launch chain — and for every image the
bits of its own one-image calls (pcl_cloud_pack_sets, pcl_trim_loss_images_sets, pcl_hist_trim_scores_images_sets,
pcl_gd_hyper.color_sets).  The colour sets are what the harness makes: ops.color_mod of each query image against the cloud's colours."""
import numpy as np
import pytest
import torch

from conftest import Cfg

pytestmark = pytest.mark.gpu

BASE = dict(max_yaw=2 * np.pi, min_yaw=0, max_pitch=2 * np.pi, min_pitch=0, max_roll=2 * np.pi, min_roll=0,
            z_prior=None, sample_rate_for_init=None, trans_init_mode="quantile",
            x_max=None, x_min=None, y_max=None, y_min=None, z_max=None, z_min=None, num_split_h=4, num_split_w=4)
STANFORD = dict(BASE, xy_only=False, num_trans=50, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4, dataset="Stanford2D-3D-S")
OMNI = dict(BASE, xy_only=True, num_trans=150, yaw_only=True, num_yaw=8, num_pitch=8, num_roll=8, dataset="OmniScenes", z_prior=0.0)


def _room(n, H, W, I, seed):
    """n-point box room, I query images of it (k/255 levels, like decoded image files) and each image's color_mod colours."""
    from piccolo_amd import ops, synth
    xyz, rgb = synth.box_room(n, seed)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    imgs, cols, poses = [], [], []
    for i in range(I):
        t_gt, ypr_gt = synth.gt_pose(seed * 10 + i)
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr_gt)), C, (H, W)))
        img_eq, rgb_eq = ops.color_mod(img, C, 256)
        imgs.append(img)
        cols.append(rgb_eq)
        poses.append((t_gt, ypr_gt))
    return X, C, imgs, cols, poses


def test_pack_sets_layout():
    from piccolo_amd import _lib, ops
    X, C, imgs, cols, _ = _room(30_000, 64, 128, 4, 3)
    one = ops.Cloud(X, C)
    sets1 = ops.Cloud.with_color_sets(X, [C], order=one.order)
    assert sets1.color_sets == 1 and torch.equal(sets1.data, one.data)
    sets = ops.Cloud.with_color_sets(X, cols, order=one.order)
    lib = _lib.load()
    plane = lib.pcl_cloud_stride(one.n)
    assert sets.data.numel() >= lib.pcl_cloud_sets_bytes(one.n, 4) == 4 * plane * (3 + 3 * 4)
    f_sets, f_one = sets.data[:4 * plane * 15].view(torch.float32), one.data[:4 * plane * 6].view(torch.float32)
    assert torch.equal(f_sets[:3 * plane], f_one[:3 * plane])
    for i, c in enumerate(cols):
        ref = ops.Cloud(X, c, order=one.order).data[:4 * plane * 6].view(torch.float32)
        assert torch.equal(f_sets[(3 + 3 * i) * plane:(6 + 3 * i) * plane], ref[3 * plane:])
    # a Cloud with sets sorts by itself like Cloud does
    assert torch.equal(ops.Cloud.with_color_sets(X, cols).order, one.order)


@pytest.mark.parametrize("I", [3, 8])
def test_trim_tables_with_color_sets_equal_single_image_tables(I):
    from piccolo_amd import ops, utils
    X, C, imgs, cols, _ = _room(120_000, 256, 512, I, 5)
    d = dict(STANFORD)
    rot = utils.generate_rot_points(d, device=X.device)
    trans = utils.generate_trans_points(X, d, device=X.device)
    groups = ops.TrimGroups(rot)
    base = ops.Cloud(X, C)
    cloud = ops.Cloud.with_color_sets(X, cols, order=base.order)
    for fmt in ("u8p", "u8"):
        panos = [ops.Pano(im, fmt=fmt) for im in imgs]
        work = ops.TrimOrder(base, (panos[0].H, panos[0].W, panos[0].fmt), trans, groups)
        for order in (None, work):
            tabs, cnts = ops.trim_loss_tables(cloud, panos, trans, groups, return_count=True, order=order)
            for i in range(I):
                t1, c1 = ops.trim_loss_table(ops.Cloud(X, cols[i], order=base.order), panos[i], trans, groups, return_count=True, order=order)
                assert torch.equal(tabs[i], t1) and torch.equal(cnts[i], c1), (fmt, order is not None, i)


@pytest.mark.parametrize("splat", [False, True])
def test_hist_scores_with_color_sets_equal_single_image_scores(splat):
    from piccolo_amd import ops, synth
    X, C, imgs, cols, poses = _room(120_000, 256, 512, 3, 7)
    base = ops.Cloud(X, C)
    cloud = ops.Cloud.with_color_sets(X, cols, order=base.order)
    K = 40
    trs, ros = [], []
    for i, (t_gt, ypr_gt) in enumerate(poses):
        tr, ro = synth.start_poses(t_gt, ypr_gt, K, seed=70 + i)
        trs.append(torch.from_numpy(tr).cuda())
        ros.append(torch.from_numpy(ro).cuda())
    scores = ops.hist_trim_scores_images(imgs, cloud, torch.stack(trs), torch.stack(ros), 4, 4, splat=splat)
    for i in range(3):
        ref = ops.hist_trim_scores(imgs[i], ops.Cloud(X, cols[i], order=base.order), trs[i], ros[i], 4, 4, splat=splat)
        assert torch.equal(scores[i], ref), i


def test_make_input_images_with_color_sets_equals_make_input():
    from piccolo_amd import utils
    X, C, imgs, cols, _ = _room(40_000, 128, 256, 4, 9)
    for init in (STANFORD, OMNI):
        single = [utils.make_input(im, X, c, 6, dict(init), "loss_histogram", 50) for im, c in zip(imgs, cols)]
        multi = utils.make_input_images(imgs, X, cols, 6, dict(init), "loss_histogram", 50)
        assert len(multi) == len(imgs)
        for (a, b), (c, e) in zip(single, multi):
            assert torch.equal(a, c) and torch.equal(b, e)


def _starts(poses, B, seed):
    from piccolo_amd import synth
    trs, ros = [], []
    for i, (t_gt, ypr_gt) in enumerate(poses):
        tr, ro = synth.start_poses(t_gt, ypr_gt, B, seed=seed + i)
        trs.append(torch.from_numpy(tr).cuda())
        ros.append(torch.from_numpy(ro).cuda())
    return trs, ros


@pytest.mark.parametrize("batch_mode", [True, False])
def test_omniloc_batch_images_with_color_sets_equals_per_image_calls(batch_mode):
    """The harness's shape (120k points, 8 candidates, 3 images), where the shared-colour plan of 24 candidates cuts the cloud into other
    chunks than the one-image plan: with colour sets every image still gets its one-image bits — graph and eager, gd_fuse on and off (at
    these shapes the chain has more blocks than are resident at once, so both take two launches per iteration; the one-launch form is
    test_fused_chain_with_color_sets_equals_per_image_calls) —, and 4 images of 5 candidates (one pose per block, where 20 candidates
    would pair them)."""
    from piccolo_amd import omniloc as po
    X, C, imgs, cols, poses = _room(120_000, 256, 512, 4, 11)
    for B, I in ((8, 3), (5, 4)):
        trs, ros = _starts(poses[:I], B, 90)
        for extra in (dict(gd_graph=True), dict(gd_graph=False), dict(gd_graph=False, gd_fuse=False), dict(gd_graph=True, gd_fuse=False)):
            cfg = Cfg(lr=0.1, num_iter=40, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B, **extra)
            t_multi, r_multi = [t.clone() for t in trs], [r.clone() for r in ros]
            multi = po.omniloc_batch_images(imgs[:I], X, cols[:I], t_multi, r_multi, cfg, batch_mode=batch_mode)
            for i in range(I):
                t1, r1 = trs[i].clone(), ros[i].clone()
                if batch_mode:
                    single = po.omniloc_batch(imgs[i], X, cols[i], t1, r1, cfg, {})
                    assert all(torch.equal(x, y) for x, y in zip(single, multi[i])), (B, extra, i)
                else:
                    res = po.omniloc_all(imgs[i], X, cols[i], t1, r1, cfg)
                    best = min(float(r[2]) for r in res)
                    assert float(multi[i][2]) == best, (B, extra, i)
                assert torch.equal(t1, t_multi[i]) and torch.equal(r1, r_multi[i]), (B, extra, i)


def _gd_plan(n, B, sets):
    """(chunks, poses per block, fused) of pcl_gd_plan_hyper for a chain of B candidates over `sets` colour sets"""
    import ctypes
    from piccolo_amd import _lib
    h = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, sets, sets)
    c, g, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.load().pcl_gd_plan_hyper(n, B, ctypes.byref(h), ctypes.byref(c), ctypes.byref(g), ctypes.byref(f)) == 0
    return c.value, g.value, f.value


@pytest.mark.parametrize("batch_mode", [True, False])
def test_fused_chain_with_color_sets_equals_per_image_calls(batch_mode):
    """The one-launch-per-iteration form (pcl_loss_fused_sets_kernel: the prologue finishes the previous iteration and reads the colour set
    from the pose records it was handed) on chains small enough to fuse: 30k points x 3 images x 8 candidates, and 20k points x 4 images x 5
    candidates (one pose per block, where the 20 candidates' shared plan would pair them).  The plan query asserts the fused form is taken;
    graph and eager, and the two-launch form of the same chain, all give every image its one-image bits."""
    from piccolo_amd import omniloc as po
    for n, B, I in ((30_000, 8, 3), (20_000, 5, 4)):
        assert _gd_plan(n, B * I, I)[2] == 1, (n, B, I)                       # every block resident: ONE launch per iteration
        assert _gd_plan(n, B * I, I) == _gd_plan(n, B, 1)
        X, C, imgs, cols, poses = _room(n, 128, 256, I, 13)
        trs, ros = _starts(poses, B, 110)
        for extra in (dict(gd_graph=True), dict(gd_graph=False), dict(gd_graph=False, gd_fuse=False)):
            cfg = Cfg(lr=0.1, num_iter=40, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B, **extra)
            t_multi, r_multi = [t.clone() for t in trs], [r.clone() for r in ros]
            multi = po.omniloc_batch_images(imgs, X, cols, t_multi, r_multi, cfg, batch_mode=batch_mode)
            for i in range(I):
                t1, r1 = trs[i].clone(), ros[i].clone()
                if batch_mode:
                    single = po.omniloc_batch(imgs[i], X, cols[i], t1, r1, cfg, {})
                    assert all(torch.equal(x, y) for x, y in zip(single, multi[i])), (n, B, extra, i)
                else:
                    res = po.omniloc_all(imgs[i], X, cols[i], t1, r1, cfg)
                    assert float(multi[i][2]) == min(float(r[2]) for r in res), (n, B, extra, i)
                assert torch.equal(t1, t_multi[i]) and torch.equal(r1, r_multi[i]), (n, B, extra, i)


def test_hist_scores_images_splat_flag_on_a_shared_cloud():
    """hist_trim_scores_images(splat=True) takes the z-buffer splat path on a cloud without colour sets too: the same scores as the
    per-image splat calls (and as the tile-binned path)."""
    from piccolo_amd import ops, synth
    X, C, imgs, _, poses = _room(60_000, 128, 256, 3, 15)
    cloud = ops.Cloud(X, C)
    trs, ros = _starts(poses, 24, 130)
    splat = ops.hist_trim_scores_images(imgs, cloud, torch.stack(trs), torch.stack(ros), 4, 4, splat=True)
    binned = ops.hist_trim_scores_images(imgs, cloud, torch.stack(trs), torch.stack(ros), 4, 4)
    assert torch.equal(splat, binned)
    for i in range(3):
        assert torch.equal(splat[i], ops.hist_trim_scores(imgs[i], cloud, trs[i], ros[i], 4, 4, splat=True)), i


def test_gd_plan_with_color_sets_is_the_single_image_plan():
    import ctypes
    from piccolo_amd import _lib
    lib = _lib.load()

    def plan(n, B, sets):
        h = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, sets, sets)
        c, g, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        assert lib.pcl_gd_plan_hyper(n, B, ctypes.byref(h), ctypes.byref(c), ctypes.byref(g), ctypes.byref(f)) == 0
        return c.value, g.value
    for n, per, I in ((120_000, 8, 3), (166_667, 6, 8), (1_000_000, 32, 5), (120_000, 5, 4)):
        assert plan(n, per * I, I) == plan(n, per, 1)
    assert plan(120_000, 24, 1) != plan(120_000, 8, 1)          # the trap: the shared-colour plan of 3 x 8 candidates differs


def test_localize_stanford_groups_images_with_per_image_colours(tmp_path, monkeypatch):
    """sharpen_color gives every image its own equalised cloud colours; with images_per_launch = 4 the three images of the room go
    through ONE make_input_images and ONE omniloc_batch_images call, and the table equals the one-by-one table bit for bit."""
    from piccolo_amd import localize
    from test_dataset_harness import COMMON, _scene, _write_stanford_tree
    root = tmp_path / "stanford"
    xyz, rgb8 = _scene()
    _write_stanford_tree(root, xyz, rgb8)
    cfg = Cfg(dataset="Stanford2D-3D-S", area=3, sharpen_color=True, **COMMON)
    table = localize.localize_stanford(cfg, None, None, root=str(root)).cpu().numpy()
    calls = []
    real_mi, real_ob = localize.make_input_images, localize.omniloc_batch_images

    def mi(imgs, xyz, rgb, *a, **k):
        calls.append(("make_input_images", len(imgs), isinstance(rgb, list)))
        return real_mi(imgs, xyz, rgb, *a, **k)

    def ob(imgs, xyz, rgb, *a, **k):
        calls.append(("omniloc_batch_images", len(imgs), isinstance(rgb, list)))
        return real_ob(imgs, xyz, rgb, *a, **k)
    monkeypatch.setattr(localize, "make_input_images", mi)
    monkeypatch.setattr(localize, "omniloc_batch_images", ob)
    again = localize.localize_stanford(Cfg(**{**cfg.__dict__, "images_per_launch": 4}), None, None, root=str(root)).cpu().numpy()
    assert calls == [("make_input_images", 3, True), ("omniloc_batch_images", 3, True)], calls
    # every column but the wall time (15), the skipped frame's NaN row included
    assert np.array_equal(again[:, :15], table[:, :15], equal_nan=True)
