"""The render + histogram stage, count for count (csrc/pcl_hist.hip; make_pano / scatter-min of csrc/pcl_ops.hip).

Everything in the stage is an integer until the last division, so on a DECISIVE scene (tests/hist_helpers.py: no point within the model's
own fp32-vs-fp64 gap x 3 of a pixel border, no two differently coloured points within that gap of each other in depth) both device
renderers must reproduce the float64 model's pixel counts exactly, its intersections within the rounding of pcl_hist_final_kernel's
arithmetic (12 x 2^-24) and its scores within that plus one rounding per slot summed.  The shapes are the ragged ones: H or W no multiple
of the split, tiles cut by the image edge, either pixel -> block mapping, the LDS 2 x 2 shortcut and the direct-to-global branch, fewer
points than a bin block, a bin-block boundary, one candidate.  On the CPU the model is anchored to the goldens (G8, G12, G19), every case
is shown to meet its caps and to give the same counts in float32 as in float64, and every case must tell the rule from its planted
variants (shifted block borders, folded remainders, farthest-wins, centre pass first, rounded colour codes, transparent black winners,
smallest index on a tie, no carry-over)."""
import numpy as np
import pytest

import hist_helpers as hh
from conftest import load_golden

gpu = pytest.mark.gpu

_SCENES, _MODELS = {}, {}


def _case(name):
    """camR1 (R1's camera-frame cloud) and R2x2 (two images on R2) are built on the shapes of R1 / R2"""
    return hh.CASES[name.replace("cam", "").split("x")[0]]


def scene(name):
    """the case's decisive scene, built once per session"""
    if name not in _SCENES:
        k = dict(_case(name))
        if name == "R2x2":                                     # two query images on R2, a second colouring for the second
            k.update(gts=2, recolor=True)
        _SCENES[name] = hh.camera_scene(**k) if name.startswith("cam") else hh.build_scene(**k)
    return _SCENES[name]


def reference(name, order=None, image=0, sets=False):
    """the float64 model of one image's candidates; order: packed slot -> point of the device's cloud (None: as given)"""
    key = (name, None if order is None else order.tobytes(), image, sets)
    if key not in _MODELS:
        sc, k = scene(name), _case(name)
        o = np.arange(len(sc.xyz)) if order is None else order
        rgb, img = (sc.rgbs[image], sc.imgs_sets[image]) if sets else (sc.rgb, sc.imgs[image])
        _MODELS[key] = hh.model(sc.xyz[o], rgb[o], img, sc.trans[image], sc.rot[image], k["nsh"], k["nsw"])
    return _MODELS[key]


ALL = hh.ROOMS + ("poles", "levels", "empty")


# ===================================================================================================== the model and the cases (CPU)
def test_model_reproduces_the_oracles_make_pano_owners_on_g8(oracle):
    g = load_golden("g8_make_pano.npz")
    H, W = [int(v) for v in g["resolution"]]
    _, owner, contested = oracle.make_pano(g["xyz_cam"], g["rgb"], (H, W), dtype=np.float64, return_aux=True)
    win = hh.render(g["xyz_cam"], g["rgb"], np.zeros(3), np.zeros(3), H, W)
    free = ~contested.ravel()
    assert free.mean() > 0.9 and np.array_equal(win[free], owner.ravel()[free])
    zmin, arg = oracle.scatter_min_depth(g["xyz_cam"], (H, W), dtype=np.float64)
    mz, marg = hh.scatter_min_model(g["xyz_cam"], H, W)
    assert np.array_equal(marg, arg) and np.allclose(mz, zmin, rtol=1e-15, atol=0)


@pytest.mark.parametrize("golden", ["g12_trim_input_hist.npz", "g19_trim_hist_empty_blocks.npz"])
def test_model_agrees_with_the_oracle_on_the_golden_scenes(oracle, golden):
    """G12 / G19 are not decisive scenes: the model (float64) and the oracle (fp32) differ by pixel-boundary flips, within the bounds that
    already hold between the oracle, the device and the reference (2e-3 on scores, 5e-2 on single blocks)"""
    from oracle import hist
    g = load_golden(golden)
    nh, nw = [int(v) for v in g["num_split"]]
    scores, slots = hist.hist_scores(g["img"], g["xyz"], g["rgb"], g["trans"], g["rot"], nh, nw)
    m = hh.model(g["xyz"], g["rgb"], g["img"], g["trans"], g["rot"], nh, nw)
    assert np.abs(m.score - scores).max() <= 2e-3, np.abs(m.score - scores).max()
    assert np.abs(m.slots - slots).max() <= 5e-2 and np.array_equal(m.slots == 0, slots == 0)
    assert np.abs(m.score - g["scores"]).max() <= 1e-2
    assert np.array_equal(hh.ranking(m.score, 4), hh.ranking(scores, 4))


@pytest.mark.parametrize("name", ALL + ("R2x2", "camR1", "camR4"))
def test_case_meets_its_caps(name):
    """caps, not measurements: at most 3 % of the points dropped, no border point and no tied pixel left; R1 keeps points inside the
    device's certificate margin (they go through the fix-up queue)"""
    sc, k = scene(name), _case(name)
    info = sc.info
    print("%s: %d of %d points kept, border %.4f, ties %d, delta %.2e px, rho %.2e" % (name, len(sc.xyz), info.n, info.border, info.tied, info.delta, info.rho))
    assert 0 < info.delta < hh.CERT_MARGIN and 0 < info.rho < 1e-5
    assert info.dropped <= hh.DROP_CAP
    border, tied = hh.undecided(sc.xyz, sc.rgb, sc.poses, sc.H, sc.W, info.delta, info.rho, sc.by_code, sc.rows)
    assert len(border) == 0 and len(tied) == 0
    if k.get("exact"):
        assert len(sc.xyz) == k["n"]
    if name == "R1":
        assert hh.near_integer(sc.xyz, sc.poses, sc.H, sc.W, info.delta, hh.CERT_MARGIN, sc.rows) >= 20


def test_cases_reach_what_they_are_there_for():
    """the paths of pcl_tile_resolve_hist_body / pcl_bin_kernel each shape is meant to take (64-pixel tiles, 2048-point bin blocks)"""
    def shape(name):
        k = hh.CASES[name]
        return k["H"], k["W"], k["H"] // k["nsh"], k["W"] // k["nsw"], len(scene(name).xyz)
    H, W, bh, bw, n = shape("R1")
    assert H < 64 and hh.CASES["R1"]["nsh"] == 3 and not (bh >= 64 and bw >= 64)
    H, W, bh, bw, n = shape("R2")
    assert bh < 64 and H % 8 == 2 and W % 5 == 2 and 64 // bh > 2 and n > 4 * 2048
    H, W, bh, bw, n = shape("R3")
    assert bw >= 64 > bh and H % 64 and W % 64 and -(-n // 2048) in (29, 30)
    H, W, bh, bw, n = shape("R4")
    assert bh >= 64 and bw >= 64 and 4 * n >= H * W
    assert shape("R5")[4] < 2048 and hh.CASES["R5"]["nsw"] == 1
    assert shape("R6a")[4] == 2049 and shape("R6b")[4] == 4096
    assert hh.CASES["R7"]["K"] == 1 and shape("R7")[0] % 2 and shape("R7")[1] % 2
    for name in hh.ROOMS:                                      # pre-dedup (4 n >= H W) has something to drop: points sharing a centre pixel
        sc = scene(name)
        r, c, _ = hh.project(hh.camera_points(sc.xyz, sc.trans[0, 0], sc.rot[0, 0], np.float64), sc.H, sc.W)
        row, col = hh.pixels(r, c, sc.H, sc.W)
        assert len(np.unique(row * sc.W + col)) < len(row)


@pytest.mark.parametrize("name", ALL)
def test_float32_model_gives_the_same_winners_and_counts(name):
    """the reference alone stays within the caps: evaluated in float32 the model decides every pixel as in float64 (the winner's colour
    code — two points of one code within rho of each other may swap, that is no tie) and counts the same histograms"""
    sc, k = scene(name), hh.CASES[name]
    m64 = reference(name)
    m32 = hh.model(sc.xyz, sc.rgb, sc.imgs[0], sc.trans[0], sc.rot[0], k["nsh"], k["nsw"], dtype=np.float32)
    scored = np.zeros(sc.H * sc.W, bool)
    scored[sc.rows[0] * sc.W:sc.rows[1] * sc.W] = True
    for i in range(k["K"]):
        assert np.array_equal(m32.wcode(i)[scored], m64.wcode(i)[scored]), i
    assert np.array_equal(m32.hist, m64.hist) and np.array_equal(m32.hist_q, m64.hist_q)
    assert np.array_equal(m32.slots, m64.slots)


@pytest.mark.parametrize("name", ALL)
def test_case_tells_the_rule_from_its_planted_variants(name):
    """a case must DIFFER from the model in an integer count under every variant its shape can reach (hist_helpers.reachable names the
    three structural exceptions); the carry-over shows in the slots"""
    sc, k = scene(name), hh.CASES[name]
    m = reference(name)
    seen = {}
    for v in hh.VARIANTS:
        mv = hh.model(sc.xyz, sc.rgb, sc.imgs[0], sc.trans[0], sc.rot[0], k["nsh"], k["nsw"], variant=v)
        if v == "no_carry":
            seen[v] = int((mv.slots != m.slots).sum())
            assert np.array_equal(mv.hist, m.hist)
        else:
            seen[v] = int((mv.hist != m.hist).sum() + (mv.hist_q != m.hist_q).sum())
    print(name, seen)
    missed = [v for v in hh.VARIANTS if hh.reachable(name, v) and not seen[v]]
    assert not missed, (name, missed)


def test_every_variant_is_reached_by_several_cases():
    for v in hh.VARIANTS:
        assert sum(hh.reachable(c, v) for c in ALL) >= (1 if v == "no_carry" else 5), v


# ===================================================================================================== the device (GPU)
@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _order(cloud, n):
    return cloud.order.cpu().numpy() if cloud.order is not None else np.arange(n, dtype=np.int64)


def _compare(parity, tag, m, dev, nsh, nsw):
    """counts as integers, intersections and scores within the arithmetic's bounds; figures printed before they are asserted"""
    s, inter, nproj, nimg = [np.asarray(v.cpu().numpy()) for v in dev]
    K = len(m.score)
    inter, nproj = inter.reshape(K, -1), nproj.reshape(K, -1)
    e_i = float(np.abs(inter.astype(np.float64) - m.inter).max())
    e_s = float(np.abs(s.astype(np.float64) - m.score).max())
    print("%s: nimg differs in %d blocks, nproj in %d of %d, |inter - model| %.3e, |score - model| %.3e" % (
        tag, int((nimg.reshape(-1) != m.nimg).sum()), int((nproj != m.nproj).sum()), nproj.size, e_i, e_s))
    assert np.array_equal(nimg.reshape(-1), m.nimg), tag
    assert np.array_equal(nproj, m.nproj), (tag, np.argwhere(nproj != m.nproj)[:8], nproj[nproj != m.nproj][:8], m.nproj[nproj != m.nproj][:8])
    parity("%s: inter vs float64 model (abs)" % tag, e_i, hh.INTER_BOUND)
    parity("%s: score vs float64 model (abs)" % tag, e_s, hh.score_bound(nsh, nsw))


def _run_case(ops, parity, name, sort, splat, batch=64):
    from piccolo_amd import omniloc as po
    sc, k = scene(name), hh.CASES[name]
    X, C, img = _t(sc.xyz), _t(sc.rgb), _t(sc.imgs[0])
    cloud = po.packed_cloud(X, C) if sort else ops.Cloud(X, C, sort=False)
    m = reference(name, _order(cloud, len(sc.xyz)))
    dev = ops.hist_trim_scores(img, cloud, _t(sc.trans[0]), _t(sc.rot[0]), k["nsh"], k["nsw"], batch=batch, return_parts=True, splat=splat)
    _compare(parity, "%s %s%s" % (name, "splat" if splat else "binned", "" if sort else " unsorted"), m, dev, k["nsh"], k["nsw"])
    return m, (X, C, img)


def _check_ranking(name, m, tensors, n_in=4):
    """utils.trim_input_hist_secondary returns the model's ranking: the best num_input scores are further apart than twice the bound"""
    from piccolo_amd import utils
    sc, k = scene(name), hh.CASES[name]
    n_in = min(n_in, k["K"])
    assert hh.separated(m.score, n_in, 2 * hh.score_bound(k["nsh"], k["nsw"])), np.sort(m.score)[::-1]
    X, C, img = tensors
    tt, tr = utils.trim_input_hist_secondary(img, X, C, _t(sc.trans[0]), _t(sc.rot[0]), n_in, k["nsh"], k["nsw"])
    best = hh.ranking(m.score, n_in)
    assert np.array_equal(tt.cpu().numpy(), sc.trans[0][best]) and np.array_equal(tr.cpu().numpy(), sc.rot[0][best])


@gpu
@pytest.mark.parametrize("splat", [False, True], ids=["binned", "splat"])
@pytest.mark.parametrize("name", hh.ROOMS + ("poles", "levels"))
def test_hist_trim_counts_equal_the_model(ops, parity, name, splat):
    m, tensors = _run_case(ops, parity, name, True, splat)
    if not splat:
        _check_ranking(name, m, tensors)


@gpu
@pytest.mark.parametrize("splat", [False, True], ids=["binned", "splat"])
def test_hist_trim_largest_packed_slot_wins_with_and_without_the_morton_sort(ops, parity, splat):
    """R1 carries exact copies of points with other colour codes: packed in the order given, the copy (the later point) wins; Morton-sorted,
    whichever of the two the sort put last — the model follows the cloud's own permutation"""
    m_sorted = _run_case(ops, parity, "R1", True, splat)[0]
    m_plain = _run_case(ops, parity, "R1", False, splat)[0]
    assert np.array_equal(m_sorted.nimg, m_plain.nimg)
    assert not np.array_equal(hh.model(scene("R1").xyz, scene("R1").rgb, scene("R1").imgs[0], scene("R1").trans[0], scene("R1").rot[0], 3, 2,
                                       variant="smallest").hist, m_plain.hist)


@gpu
@pytest.mark.parametrize("splat", [False, True], ids=["binned", "splat"])
@pytest.mark.parametrize("batch", [16, 5, 1])
def test_hist_trim_carry_over_crosses_batch_boundaries(ops, parity, batch, splat):
    m, tensors = _run_case(ops, parity, "empty", True, splat, batch=batch)
    assert (m.nproj[1:, 0] == 0).any() and (m.slots[1:, 3] > 0).any()             # a carried, non-zero slot behind an empty block
    if not splat and batch == 16:
        _check_ranking("empty", m, tensors)


@gpu
@pytest.mark.parametrize("splat", [False, True], ids=["binned", "splat"])
@pytest.mark.parametrize("sets", [False, True], ids=["shared", "sets"])
def test_hist_trim_images_equal_the_model(ops, parity, sets, splat):
    """two query images on R2 in one set of launches, with the cloud's colours and with a colour set per image: every image against the
    model of its own candidates (and its own carry-over chain), not against the one-image call"""
    import torch
    sc, k = scene("R2x2"), hh.CASES["R2"]
    X = _t(sc.xyz)
    cloud = ops.Cloud.with_color_sets(X, [_t(c) for c in sc.rgbs]) if sets else ops.Cloud(X, _t(sc.rgb))
    order = _order(cloud, len(sc.xyz))
    imgs = [_t(im) for im in (sc.imgs_sets if sets else sc.imgs)]
    trans, rot, K = _t(sc.trans), _t(sc.rot), k["K"]
    scores = ops.hist_trim_scores_images(imgs, cloud, trans, rot, k["nsh"], k["nsw"], splat=splat)
    # (the counts behind the scores: the driver that hist_trim_scores_images hands its arguments to)
    s2, inter, nproj, nimg = ops._hist_scores("hist_trim_scores_images", imgs, cloud, trans, rot, k["nsh"], k["nsw"], splat)
    assert torch.equal(scores, s2)
    for i in range(2):
        m = reference("R2x2", order, image=i, sets=sets)
        tag = "R2 x 2 images%s %s, image %d" % (" (sets)" if sets else "", "splat" if splat else "binned", i)
        _compare(parity, tag, m, (scores[i], inter[i * K:(i + 1) * K], nproj[i * K:(i + 1) * K], nimg[i]), k["nsh"], k["nsw"])


@gpu
@pytest.mark.parametrize("name", ["camR1", "camR4"])
def test_make_pano_and_scatter_min_equal_the_model_in_every_pixel(ops, name):
    """the stand-alone ops on a decisive camera-frame cloud: the same key rule (make_pano: latest pass, nearest, largest index; scatter-min:
    nearest, smallest index), every pixel"""
    sc = scene(name)
    H, W = sc.H, sc.W
    img = ops.make_pano(_t(sc.xyz), _t(sc.rgb), (H, W)).cpu().numpy().reshape(H * W, 3)
    win = hh.render(sc.xyz, sc.rgb, np.zeros(3), np.zeros(3), H, W)
    want = np.where((win >= 0)[:, None], (sc.rgb * np.float32(255))[np.maximum(win, 0)], np.float32(0))
    print("%s: make_pano differs in %d of %d pixels" % (name, int((img != want).any(axis=1).sum()), H * W))
    assert np.array_equal(img, want)
    for edge in (win[:W], win[-W:], win[::W], win[W - 1::W]):                  # the clamped footprints are there
        assert (edge >= 0).any()
    zmin, arg = ops.scatter_min_depth(_t(sc.xyz), (H, W))
    mz, marg = hh.scatter_min_model(sc.xyz, H, W)
    zmin, arg = zmin.cpu().numpy().astype(np.float64), arg.cpu().numpy()
    print("%s: scatter-min argmin differs in %d pixels, depth by %.3e (relative)" % (name, int((arg != marg).sum()), float((np.abs(zmin - mz)[mz > 0] / mz[mz > 0]).max())))
    assert np.array_equal(arg, marg)
    assert (np.abs(zmin - mz) <= sc.info.rho * mz).all()
