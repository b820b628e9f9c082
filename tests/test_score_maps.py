"""Score maps (csrc/pcl_score.hip): per image patch and per point, the histogram stage's patch intersections averaged over the candidate
poses, and the weight plane made from the per-point map.  Build-defined (include/piccolo_hip.h); the rules are restated by the plain numpy
model of tests/score_helpers.py.

On the CPU the model is shown to tell the rules from four planted variants (a mean over all K poses, unscored rows folded into the nearest
scored row, the remainder column folded into the last block, a vote counted although its block is invalid) on hist_helpers' decisive
scenes R1, R2, R5, R6a and `empty`, whose points have the same block in float32 as in float64 for every pose.  On the GPU both maps must
equal the model bit for bit when the model is fed the device's own histogram parts (that stage is pinned by test_hist_exact.py): only
the new arithmetic is under test.  With 300 poses on R1's cloud the scene is no longer decisive; there every DECIDED point (no float64
pixel coordinate within 3 x the model's own fp32-vs-fp64 gap of a block border) is compared bit for bit and the undecided share is capped."""
import numpy as np
import pytest

import hist_helpers as hh
import score_helpers as sh
from conftest import Cfg

gpu = pytest.mark.gpu

_BLOCKS, _PARTS = {}, {}
MANY = dict(K=300, splits=((7, 8), (3, 2)))


def blocks(name, dtype=np.float64, variant=None):
    key = (name, np.dtype(dtype).name, variant)
    if key not in _BLOCKS:
        sc, k = sh.scene(name), hh.CASES[name]
        _BLOCKS[key] = sh.point_blocks(sc.xyz, sc.trans[0], sc.rot[0], k["H"], k["W"], k["nsh"], k["nsw"], dtype, variant)
    return _BLOCKS[key]


def parts(name):
    """the float64 model's inter, nproj, nimg of the case (the CPU tests' stand-in for the device's parts)"""
    if name not in _PARTS:
        sc, k = sh.scene(name), hh.CASES[name]
        m = hh.model(sc.xyz, sc.rgb, sc.imgs[0], sc.trans[0], sc.rot[0], k["nsh"], k["nsw"])
        _PARTS[name] = (m.inter.astype(np.float32), m.nproj, m.nimg)
    return _PARTS[name]


def many_poses():
    from piccolo_amd import synth
    sc = sh.scene("R1")
    return synth.start_poses(sc.gt[0][0], sc.gt[1][0], MANY["K"], seed=7, sigma_t=0.5, sigma_r=0.4)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_maps(a, b):
    return all(np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))) for f in ("score3d", "count3d", "score2d", "count2d"))


# ===================================================================================================== the model and the cases (CPU)
@pytest.mark.parametrize("name", sh.CASE_NAMES)
def test_float32_and_float64_give_every_point_the_same_block(name):
    assert np.array_equal(blocks(name), blocks(name, np.float32))


def test_cases_reach_what_they_are_there_for():
    counts = {}
    for name in sh.CASE_NAMES:
        inter, nproj, nimg = parts(name)
        m = sh.maps_model(blocks(name), inter, nproj, nimg)
        counts[name] = m.count3d
        assert m.count3d.min() >= 0 and m.count3d.max() <= 9
        assert np.array_equal(m.score3d == -1, m.count3d == 0) and np.array_equal(m.score2d == -1, m.count2d == 0)
        assert (m.score3d[m.count3d > 0] >= 0).all() and (m.score3d <= 1).all()
    every = np.concatenate(list(counts.values()))
    assert set(np.unique(every)) == set(range(10))                       # counts range over 0 .. 9
    assert (counts["R1"] == 0).any() and (counts["R5"] == 0).any()        # points with no vote
    for name in ("R2", "empty"):                                          # invalid blocks
        _, nproj, nimg = parts(name)
        assert ((nproj == 0) | (nimg[None] == 0)).any(), name


def reachable(name, variant):
    """Can the case tell `variant` from the rule at all?  fold_cols: only with a column remainder a centre pixel can lie in — at least two
    columns wide, because the image's last column is the centre pixel of a point at column coordinate W - 1 exactly and of no other (R1
    and `empty`, 129 = 2 x 64 + 1, have that one column only; of the five cases R2 alone has two); count_invalid: only where a point falls
    into an invalid block — a block without rendered pixels rarely holds a centre pixel (R2's one invalid block holds none); `empty`, whose
    query image is black where its candidates see the wall, is the case for it.  The other two must show in every case."""
    k = hh.CASES[name]
    if variant == "fold_cols":
        return k["W"] - k["nsw"] * (k["W"] // k["nsw"]) >= 2
    if variant == "count_invalid":
        _, nproj, nimg = parts(name)
        blk, valid = blocks(name), (nproj > 0) & (nimg[None] > 0)
        return bool(((blk >= 0) & ~np.take_along_axis(valid, np.maximum(blk, 0), axis=1)).any())
    return True


@pytest.mark.parametrize("name", sh.CASE_NAMES)
def test_case_tells_the_rule_from_its_planted_variants(name):
    inter, nproj, nimg = parts(name)
    rule = sh.maps_model(blocks(name), inter, nproj, nimg)
    for variant in sh.VARIANTS:
        if not reachable(name, variant):
            continue
        v = sh.maps_model(blocks(name, variant=variant), inter, nproj, nimg, variant)
        assert not (np.array_equal(v.score3d, rule.score3d) and np.array_equal(v.count3d, rule.count3d)), (name, variant)
        if variant == "all_k" and name in ("R2", "empty"):
            assert not np.array_equal(v.score2d, rule.score2d), name


def test_every_variant_is_reached():
    reached = {variant: [name for name in sh.CASE_NAMES if reachable(name, variant)] for variant in sh.VARIANTS}
    assert reached["fold_cols"] == ["R2"] and "empty" in reached["count_invalid"]
    assert reached["all_k"] == list(sh.CASE_NAMES) and reached["fold_rows"] == list(sh.CASE_NAMES)


@pytest.mark.parametrize("split", MANY["splits"])
def test_many_poses_undecided_share_is_under_its_cap(split):
    sc, k = sh.scene("R1"), hh.CASES["R1"]
    trans, rot = many_poses()
    und, delta, flips = sh.undecided_points(sc.xyz, trans, rot, k["H"], k["W"], *split)
    print("split %d x %d: delta %.3e, undecided %.2f %% of %d points, float32 flips among the decided %d" % (*split, delta, 100 * und.mean(), len(und), flips))
    assert und.mean() <= sh.UNDECIDED_CAP and flips == 0


def test_weight_model_basics():
    s, c = np.array([0.2, 0.6, 0.4, -1.0, 0.9], np.float32), np.array([3, 9, 5, 0, 1])
    plane, rng = sh.weights_model(s, c, 0.0, 1, 8)
    q = lambda v: (np.float32(v) - np.float32(0.2)) / (np.float32(0.9) - np.float32(0.2))      # noqa: E731
    assert np.array_equal(plane, np.array([0, q(0.6), q(0.4), 1, 1, 0, 0, 0], np.float32)) and rng[2] == 4
    plane, rng = sh.weights_model(s, c, 0.25, 5, 8)
    assert plane[0] == 1 and plane[1] == 1 and plane[2] == np.float32(0.25) and plane[3] == 1 and plane[4] == 1 and rng == (np.float32(0.4), np.float32(0.6), 2)
    assert np.array_equal(sh.weights_model(s, np.zeros(5, int), 0.0, 1, 8)[0], np.array([1, 1, 1, 1, 1, 0, 0, 0], np.float32))
    assert np.array_equal(sh.weights_model(np.full(5, 0.5, np.float32), c, 0.5, 1, 8)[0], np.array([1, 1, 1, 1, 1, 0, 0, 0], np.float32))
    x = np.random.default_rng(0).random(2000).astype(np.float32)
    a, f = np.float32(0.75), np.float32(0.25)
    assert np.array_equal(sh.fma32(a, x, f), np.array([np.float32(float(a) * float(v) + float(f)) for v in x]))   # (no half-way sum among them)


# ===================================================================================================== the device (GPU)
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


def host(t):
    return t.cpu().numpy()


def _order(cloud, n):
    return host(cloud.order) if cloud.order is not None else np.arange(n, dtype=np.int64)


def _device_maps(ops, cloud, img, trans, rot, nsh, nsw, packed):
    import types
    H, W = int(img.shape[0]), int(img.shape[1])
    _, inter, nproj, nimg = ops.hist_trim_scores(img, cloud, T(trans), T(rot), nsh, nsw, return_parts=True)
    s3, c3, s2, c2 = ops.score_maps(cloud, T(trans), T(rot), H, W, nsh, nsw, inter, nproj, nimg, packed=packed)
    K = len(trans)
    dev = types.SimpleNamespace(score3d=host(s3), count3d=host(c3), score2d=host(s2), count2d=host(c2))
    return dev, (host(inter).reshape(K, -1), host(nproj).reshape(K, -1), host(nimg).reshape(-1)), (s3, c3)


@gpu
@pytest.mark.parametrize("sort", [True, False], ids=["morton", "unsorted"])
@pytest.mark.parametrize("name", sh.CASE_NAMES)
def test_maps_equal_the_model_bit_for_bit(ops, name, sort):
    sc, k = sh.scene(name), hh.CASES[name]
    n = len(sc.xyz)
    cloud = ops.Cloud(T(sc.xyz), T(sc.rgb), sort=sort)
    order = _order(cloud, n)
    assert sort == (cloud.order is not None)
    for packed in (True, False):
        dev, (inter, nproj, nimg), _ = _device_maps(ops, cloud, T(sc.imgs[0]), sc.trans[0], sc.rot[0], k["nsh"], k["nsw"], packed)
        blk = blocks(name)[:, order] if packed else blocks(name)
        m = sh.maps_model(blk, inter, nproj, nimg)
        tag = "%s %s %s" % (name, "morton" if sort else "unsorted", "packed" if packed else "caller order")
        print("%s: score3d differs at %d of %d points, count3d at %d, score2d at %d of %d blocks, count2d at %d; counts %d .. %d" % (
            tag, int((bits(dev.score3d) != bits(m.score3d)).sum()), n, int((dev.count3d != m.count3d).sum()),
            int((bits(dev.score2d) != bits(m.score2d)).sum()), len(m.score2d), int((dev.count2d != m.count2d).sum()), m.count3d.min(), m.count3d.max()))
        assert dev.count3d.dtype == np.int32 and dev.count2d.dtype == np.int32 and dev.score3d.dtype == np.float32
        assert same_maps(dev, m), tag
    if name == "R1":                                                      # a pose that is not finite casts no vote; either output pair alone
        import torch
        trans = sc.trans[0].copy()
        trans[4, 1] = np.nan
        dev, (inter, nproj, nimg), _ = _device_maps(ops, cloud, T(sc.imgs[0]), trans, sc.rot[0], k["nsh"], k["nsw"], False)
        m = sh.maps_model(sh.point_blocks(sc.xyz, trans, sc.rot[0], k["H"], k["W"], k["nsh"], k["nsw"]), inter, nproj, nimg)
        assert same_maps(dev, m) and m.count3d.max() <= 8
        lib, K, nblk = ops._lib.load(), 9, (k["nsh"] - 2) * k["nsw"]
        nws = lib.pcl_score_maps_workspace_bytes(n, K, k["nsh"], k["nsw"])
        ws, s3, c3 = ops._bytes(nws), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        s2, c2 = torch.empty(nblk, device="cuda"), torch.empty(nblk, dtype=torch.int32, device="cuda")
        keep = [T(trans), T(sc.rot[0]), T(inter), T(nproj), T(nimg)]     # (alive until the calls have run)
        args = (ops._ptr(cloud.data), n, ops._ptr(keep[0]), ops._ptr(keep[1]), K, k["H"], k["W"], k["nsh"], k["nsw"], ops._ptr(keep[2]),
                ops._ptr(keep[3]), ops._ptr(keep[4]), ops._ptr(cloud.order))
        assert lib.pcl_score_maps(*args, ops._ptr(s3), ops._ptr(c3), None, None, ops._ptr(ws), nws, ops._stream()) == 0
        assert lib.pcl_score_maps(*args, None, None, ops._ptr(s2), ops._ptr(c2), ops._ptr(ws), nws, ops._stream()) == 0
        assert np.array_equal(bits(host(s3)), bits(m.score3d)) and np.array_equal(host(c3), m.count3d)
        assert np.array_equal(bits(host(s2)), bits(m.score2d)) and np.array_equal(host(c2), m.count2d)


@gpu
@pytest.mark.parametrize("split", MANY["splits"])
def test_many_poses_every_decided_point_bit_for_bit(ops, split):
    sc, k = sh.scene("R1"), hh.CASES["R1"]
    trans, rot = many_poses()
    und, delta, _ = sh.undecided_points(sc.xyz, trans, rot, k["H"], k["W"], *split)
    print("split %d x %d: undecided %.2f %% of %d points (delta %.3e)" % (*split, 100 * und.mean(), len(und), delta))
    assert und.mean() <= sh.UNDECIDED_CAP
    cloud = ops.Cloud(T(sc.xyz), T(sc.rgb))
    dev, (inter, nproj, nimg), _ = _device_maps(ops, cloud, T(sc.imgs[0]), trans, rot, *split, False)
    m = sh.maps_model(sh.point_blocks(sc.xyz, trans, rot, k["H"], k["W"], *split), inter, nproj, nimg)
    dec = ~und
    print("decided points that differ: score %d, count %d; counts %d .. %d" % (
        int((bits(dev.score3d) != bits(m.score3d))[dec].sum()), int((dev.count3d != m.count3d)[dec].sum()), m.count3d.min(), m.count3d.max()))
    assert np.array_equal(bits(dev.score3d)[dec], bits(m.score3d)[dec]) and np.array_equal(dev.count3d[dec], m.count3d[dec])
    assert np.array_equal(bits(dev.score2d), bits(m.score2d)) and np.array_equal(dev.count2d, m.count2d)


@gpu
def test_weight_plane_equals_the_model_bit_for_bit(ops):
    import torch
    from piccolo_amd import omniloc as po
    sc, k = sh.scene("R1"), hh.CASES["R1"]
    n = len(sc.xyz)
    X, C, img = T(sc.xyz), T(sc.rgb), T(sc.imgs[0])
    cloud = po.packed_cloud(X, C)
    stride = ops._lib.load().pcl_cloud_stride(n)
    assert stride > n                                                     # (there is padding to check)
    dev, _, (s3, c3) = _device_maps(ops, cloud, img, sc.trans[0], sc.rot[0], k["nsh"], k["nsw"], True)
    assert (dev.count3d >= 5).any() and (dev.count3d < 5).any() and (dev.count3d == 0).any()
    flat = np.where(dev.count3d > 0, np.float32(0.375), np.float32(-1))
    cases = [(dev.score3d, dev.count3d, f, mc) for f in (0.0, 0.25) for mc in (1, 5)]
    cases += [(dev.score3d, np.zeros(n, np.int32), 0.25, 1), (flat, dev.count3d, 0.25, 1)]
    for score, count, floor, min_count in cases:
        plane, rng = ops.score_weight_plane(n, T(score), T(count), floor, min_count)
        want, (lo, hi, voted) = sh.weights_model(score, count, floor, min_count, stride)
        got = host(plane)
        print("floor %.2f min_count %d: plane differs at %d of %d slots; lo %.6f hi %.6f voted %d; weights %.4f .. %.4f" % (
            floor, min_count, int((bits(got) != bits(want)).sum()), stride, lo, hi, voted, want[:n].min(), want[:n].max()))
        assert np.array_equal(bits(got), bits(want)) and (got[n:] == 0).all()
        assert np.array_equal(bits(host(rng)), bits(np.array([lo, hi, voted], np.float32)))
    # the surface: weights in the caller's order, and the plane Cloud.set_weights packs from them is the plane of the packed map
    maps = po.score_maps(img, X, C, T(sc.trans[0]), T(sc.rot[0]), k["nsh"], k["nsw"])
    assert maps.score2d.shape == (k["nsh"] - 2, k["nsw"]) and maps.count2d.shape == maps.score2d.shape
    order = _order(cloud, n)
    assert np.array_equal(bits(host(maps.score3d)[order]), bits(dev.score3d)) and np.array_equal(host(maps.count3d)[order], dev.count3d)
    w = po.score_weights(maps, floor=0.25, min_count=5)
    assert w.shape == (n,)
    packed_plane, _ = ops.score_weight_plane(n, s3, c3, 0.25, 5)
    c = ops.Cloud(X, C, order=cloud.order)
    c.set_weights(w)
    assert torch.equal(c.weights, packed_plane)
    for bad in (ops.Cloud(X, C, weights=torch.ones(n)), ops.Cloud.with_color_sets(X, [C, C])):
        with pytest.raises(ValueError):
            ops.score_maps(bad, T(sc.trans[0]), T(sc.rot[0]), k["H"], k["W"], k["nsh"], k["nsw"], maps.inter, maps.nproj, maps.nimg)
    with pytest.raises(ValueError):
        ops.score_weight_plane(n, s3, c3, floor=1.0)
    with pytest.raises(ValueError):
        ops.score_weight_plane(n, s3, c3, min_count=0)


def _room(n=20_000, H=128, W=256, seed=3):
    from piccolo_amd import ops, synth
    xyz, rgb = synth.box_room(n, seed)
    t_gt, ypr_gt = synth.gt_pose(seed)
    X, C = T(xyz), T(rgb)
    cam = ops.transform_cloud(X, T(t_gt), T(ypr_gt))
    return X, C, synth.quantise_like_image_file(ops.make_pano(cam, C, (H, W))), (t_gt, ypr_gt)


INIT = dict(max_yaw=2 * np.pi, min_yaw=0, max_pitch=2 * np.pi, min_pitch=0, max_roll=2 * np.pi, min_roll=0, z_prior=None, sample_rate_for_init=None,
            trans_init_mode="quantile", x_max=None, x_min=None, y_max=None, y_min=None, z_max=None, z_min=None, num_split_h=4, num_split_w=4,
            xy_only=False, num_trans=50, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4, dataset="Stanford2D-3D-S")


@gpu
def test_make_input_scored_keeps_make_inputs_poses_and_the_histogram_parts(ops):
    import torch
    from piccolo_amd import omniloc as po, utils
    X, C, img, _ = _room()
    init = dict(INIT)
    want_t, want_r = utils.make_input(img, X, C, 4, init, "loss_histogram", 12)
    tt, tr, maps = utils.make_input_scored(img, X, C, 4, init, "loss_histogram", 12)
    assert torch.equal(tt, want_t) and torch.equal(tr, want_r)
    # the maps are taken over the survivors of the loss trim, at the initialisation's own split
    t1, r1 = utils.trim_input_loss(img, X, C, *utils.candidate_grids(img, X, init), 12)
    ref = po.score_maps(img, X, C, t1, r1, init["num_split_h"], init["num_split_w"])
    for f in ("score3d", "count3d", "score2d", "count2d", "inter", "nproj", "nimg"):
        assert torch.equal(getattr(maps, f), getattr(ref, f)), f
    assert int(maps.count3d.max()) > 0
    _, _, other = utils.make_input_scored(img, X, C, 4, init, "loss_histogram", 12, score_split=(8, 6))
    assert other.score2d.shape == (6, 6) and other.score3d.shape == maps.score3d.shape and int(other.count3d.max()) > 0


@gpu
def test_refinement_under_score_weights_is_the_weighted_chain(ops):
    import torch
    from piccolo_amd import omniloc as po, synth
    X, C, img, (t_gt, ypr_gt) = _room()
    n = X.shape[0]
    trans, rot = synth.start_poses(t_gt, ypr_gt, 6, seed=5)
    maps = po.score_maps(img, X, C, T(trans), T(rot), 4, 4)
    w = po.score_weights(maps, floor=0.25)
    assert float(w.min()) < 1.0 and float(w.max()) == 1.0
    cfg = Cfg(lr=0.1, num_iter=12, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=6)
    t, R, loss = po.omniloc_batch(img, X, C, T(trans.copy()), T(rot.copy()), cfg, {}, weights=w)
    cloud = po.packed_cloud(X, C)
    order = _order(cloud, n)
    plane, _ = ops.score_weight_plane(n, maps.score3d[T(order)], maps.count3d[T(order)], 0.25)
    gd = ops.GradientDescent(cloud.weighted_view(plane), po.packed_pano(img, n_points=n), T(trans), T(rot), po.quantile_box_of(X, 0.05), lr=0.1,
                             patience=5, factor=0.8, batch_mode=True)
    gd.run(12)
    want = gd.winner(1)[0].cpu()
    assert torch.equal(t.reshape(3), want[0:3]) and torch.equal(R.reshape(9), want[3:12]) and torch.equal(loss.reshape(1), want[12:13])
    plain = po.omniloc_batch(img, X, C, T(trans.copy()), T(rot.copy()), cfg, {})
    assert not torch.equal(plain[2], loss)                                # the weights matter


@gpu
def test_stanford_loop_under_score_weights_runs_the_scored_path(ops, tmp_path, monkeypatch):
    """cfg.score_weights: every image that is not skipped is initialised with make_input_scored at cfg.score_split and refined through
    refine_image under omniloc.score_weights of its maps; the table's shape, the CSV's header and the skipped row stay as they are"""
    import csv
    import test_dataset_harness as dh
    from piccolo_amd import localize, omniloc as po
    root = tmp_path / "stanford"
    xyz, rgb8 = dh._scene()
    dh._write_stanford_tree(root, xyz, rgb8)
    seen = []
    scored, refine = localize.make_input_scored, localize.refine_image

    def make_input_scored(*args, **kw):
        out = scored(*args, **kw)
        seen.append(["init", kw.get("score_split"), out[2]])
        return out

    def refine_image(img, X, C, tr, ro, cfg, scalar_summaries=None, weights=None):
        seen.append(["refine", weights])
        return refine(img, X, C, tr, ro, cfg, scalar_summaries, weights=weights)

    monkeypatch.setattr(localize, "make_input_scored", make_input_scored)
    monkeypatch.setattr(localize, "refine_image", refine_image)
    cfg = Cfg(dataset="Stanford2D-3D-S", area=3, sharpen_color=True, score_weights=True, score_split=[8, 8], score_floor=0.25, **dh.COMMON)
    log = tmp_path / "log"
    table = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
    assert table.shape == (4, 16) and np.isnan(table[2]).all() and not np.isnan(table[[0, 1, 3]]).any()
    assert [s[0] for s in seen] == ["init", "refine"] * 3
    for init, ref in zip(seen[0::2], seen[1::2]):
        maps, w = init[2], ref[1]
        assert init[1] == (8, 8) and maps.score2d.shape == (6, 8) and w is not None and w.shape == (len(xyz),)
        assert bool((w == po.score_weights(maps, 0.25, 1)).all()) and float(w.min()) >= 0.25 and float(w.max()) == 1.0
    assert (table[:2, 13] < 0.2).all() and (table[:2, 14] < 5.0).all(), table[:, 13:15]
    with open(log / "stanford_results.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == localize.STANFORD_HEADER and [r[4] for r in rows[1:]] == ["0", "0", "1", "0"]
