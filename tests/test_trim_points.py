"""The trim kernel pair by pair against a float64 model (tests/trim_helpers.py).

A cloud of one point under K translations and R rotations returns every (translation, rotation) pair's own term in one
trim_loss_table launch: every class size, padded yaw slots, the seam, the poles, the zero border, black taps, points next to the camera's
vertical axis, all texel layouts.  Clouds of distinct points fill every lane and both packed halves; several images per launch go through
colour sets and the work list.  The CPU part holds the share of pairs left out under its cap by the models alone and shows that each
planted mistake of the kernel's formula breaks the bound the device is held to."""
import numpy as np
import pytest

import grad_helpers as gh
import trim_helpers as th

gpu = pytest.mark.gpu

CASES = th.one_point_cases()
U = 2.0 ** -24

# Cases whose border pairs are lattice coincidences of the construction itself, not of the rule: a target that sits on the fraction 0.5 of a
# texel lands ON a texel centre under another member of the table (300 x 100 under the eight yaws: a yaw step is 12.5 px; the quarter
# turns of the 3-DoF grid map half-texel targets of 64 x 128 and 300 x 100 onto rows / columns likewise).  Asserted below: every border
# pair of these cases is such a coincidence; every other case stays under gh.BORDER_CAP.
LATTICE = {("border300", "probe", "yaw8"), ("border300", "probe", "stanford"), ("black", "probe", "stanford")}


# ============================================================================================= the tables, the rule (CPU)
def test_rotation_tables_have_the_classes_they_are_for():
    st, y8, rg = (th.classes(th.table(t)) for t in th.TABLES)
    assert len(th.table("stanford")) == 24 and st["sizes"] == [4] * 6 and len(st["groups"]) == 6
    assert y8["sizes"] == [8] and [len(m) for _, m in y8["groups"]] == [4, 4]
    assert rg["sizes"] == th.RAGGED_SIZES and sorted(len(m) for _, m in rg["groups"]) == [1, 1, 2, 3, 4]
    rot = th.table("ragged")
    assert (rot[:, 0] < 0).any() and (rot[:, 0] > 2 * np.pi).any()
    z = rg["M"][:, 2]
    near = sorted(float(np.abs(z[i] - z[j]).max()) for i in range(len(rot)) for j in range(i) if 0 < np.abs(z[i] - z[j]).max() < 1e-5)
    assert len(near) == 3 and 0 < near[0] < th.TOL < near[1]            # one merged pair, and the single rotation apart from both of it
    # yaws 0, pi / 2, pi, 3 pi / 2 relative to each class's first rotation
    d = np.sort(np.mod(st["delta"].reshape(-1)[np.argsort(st["leader"], kind="stable")].reshape(6, 4), 2 * np.pi), 1)
    assert np.abs(d - np.arange(4) * np.pi / 2).max() < 1e-6


@pytest.mark.parametrize("c", CASES, ids=th.case_id)
def test_border_and_seam_share(oracle, c):
    """by the models alone: border plus seam pairs are at most 1 % of a case's pairs, no aimed probe is one, and the case holds what
    it is for"""
    k = th.case(c)
    name, pano, tb = c
    for flt in (False, True):
        if flt and pano == "lv1024":
            continue
        ru = th.rule(oracle, c, flt)
        n, out = len(ru["ok"]), int((~ru["ok"]).sum())
        print("%s flt=%d: %d pairs, border %d, seam %d (%d to the generic kernel), masked %d: %.2f %% left out; gap %.2e px"
              % (th.case_id(c), flt, n, ru["border"].sum(), ru["seam"].sum(), ru["seam_ok"].sum(), (~ru["kept"]).sum(), 100.0 * out / n, ru["gap"]))
        assert not (k["aimed"].reshape(-1) & ~ru["ok"]).any(), "an aimed pair is not decisive"
        # (the poles under yaw-only rotations: every pair inside the cone around the axis, each with its own gap, no common delta)
        assert (0 < ru["delta"] or (name, tb) == ("poles", "yaw8")) and ru["delta"] <= 3 * 4 * max(ru["H"], ru["W"]) * 2.0 ** -23
        if c in LATTICE:
            tt, rr = th.pairs(k["trans"], k["rot"])
            m = gh.model(oracle, k["x"][None, :], k["rgb"][None, :], k["imgf"] if flt else k["img"], tt, rr, np.float64)
            on = np.minimum(np.abs(m["ix"] - np.round(m["ix"])), np.abs(m["iy"] - np.round(m["iy"]))) < ru["delta"]
            assert (on | ~ru["border"]).all() and np.array_equal(ru["kept"], ru["kept32"]) and out <= 0.041 * n
        else:
            assert out <= gh.BORDER_CAP * n, (c, out, n)
    ru = th.rule(oracle, c)
    H = ru["H"]
    if name == "poles":
        yb = ru["y0"][k["aimed"].reshape(-1)] + 1                  # rows of the bordered texture
        # the clip at +-0.99 ends the rows at floor(0.995 H + 0.5) (64: the last row, H; 127: H - 1) and at 0 or 1
        assert yb.max() == int(np.floor(0.995 * H + 0.5)) == (H if H == 64 else H - 1) and yb.min() == int(np.floor(0.005 * H + 0.5))
    if name == "random" or c[1] == "lv127":
        assert ((ru["y0"][ru["ok"]] + 1) % 2 == 0).any() and ((ru["y0"][ru["ok"]] + 1) % 2 == 1).any()
    if name == "black":
        assert (~ru["kept"] & k["aimed"].reshape(-1)).sum() >= 6 * len(k["rot"])
    if name == "seam":
        assert ru["seam_ok"].sum() >= 9
    if name == "near_axis":
        rho2 = ru["rho"] ** 2
        assert (rho2 < th.TINY_OLD).any() and ((rho2 > th.TINY_OLD) & (rho2 < th.TINY)).sum() > 0.25 * len(rho2) and (rho2 > th.TINY).any()
    if name == "random":
        assert (~ru["kept"]).any() and ru["kept"].sum() > 0.8 * len(ru["kept"])


# ======================================================================================================= planted variants (CPU)
def _near(ru):
    return (ru["rho"] >= 1.04e-4) & (ru["rho"] <= 5.05e-4)


def _last_column(R):
    return lambda ru: np.arange(len(ru["ok"])) % R == R - 1


def _merged_pair(ru):
    """the pairs of the ragged table's rotation that joined a class through the tolerance (row 6)"""
    return np.arange(len(ru["ok"])) % 11 == 6


# variant -> [(case, which pairs it is about (None: all decisive pairs))]
CATCHERS = {
    "no_carry": [(("rho", "probe", "stanford"), None), (("near_axis", "lv64", "yaw8"), None)],
    "first_order": [(("near_axis", "lv64", "stanford"), _near), (("near_axis", "lv64", "yaw8"), _near), (("near_axis", "lv1024", "yaw8"), _near)],
    "seam_sum": [(("seam", "probe", t), "seam") for t in th.TABLES],
    "pair_row": [(("random", "lv127", "stanford"), None), (("poles", "lv127", "ragged"), None)],
    "rot_idx": [(("random", "lv64", "stanford"), None), (("random", "lv16", "ragged"), None), (("random", "lv300", "yaw8"), None)],
    "padded_slot": [(("random", "lv64", "ragged"), _last_column(11)), (("fractions", "probe", "ragged"), _last_column(11))],
    "black_tap": [(("black", "probe", "stanford"), None), (("black", "probe", "ragged"), None)],
    "merged_row": [(("axis", "probe", "stanford"), None), (("poles", "lv127", "stanford"), None), (("axis", "probe", "ragged"), _merged_pair)],
}


def _seam_breaks(ru, loss, kept):
    """at the seam pairs the reference is the fp32 evaluation (on the device: the generic kernel): the same end, the same bound"""
    sel = ru["seam_ok"]
    if not np.array_equal(kept[sel], ru["kept32"][sel]):
        return True
    sel = sel & ru["kept32"]
    s = float(np.median(ru["l64"][ru["ok"] & ru["kept"]]))
    return gh.exceeds(gh.three_stats(th.errors(loss, ru["l32"], sel, s)), th.yardstick(ru))


@pytest.mark.parametrize("variant", list(th.VARIANTS))
def test_planted_variants_break_the_bound(oracle, variant):
    """each planted mistake of the kernel's formula is further from the model than the device may be, on the pairs it is about — and the
    formula without a mistake is not, on the same pairs"""
    for c, which in CATCHERS[variant]:
        k, ru = th.case(c), th.rule(oracle, c)
        good, bad = th.emulate(oracle, k, k["img"]), th.emulate(oracle, k, k["img"], variant)
        if which == "seam":
            assert ru["seam_ok"].any() and not _seam_breaks(ru, *good), c
            assert _seam_breaks(ru, *bad), (th.VARIANTS[variant], c)
            continue
        sel = None if which is None else which(ru)
        assert sel is None or (sel & ru["ok"] & ru["kept"]).sum() >= 20, c
        assert not th.breaks(ru, *good, sel=sel), c
        assert th.breaks(ru, *bad, sel=sel), (th.VARIANTS[variant], c)


@pytest.mark.parametrize("c", CASES, ids=th.case_id)
def test_the_formula_with_the_derived_thresholds_holds_the_bound(oracle, c):
    """the kernel's formula in float64 — the exact branch up to rho^2 = th.TINY, a merged class's correction within th.MERGE_CONE of the
    axis — is within the device's bound of the model on the decisive pairs of every case and at its seam pairs; with the old threshold
    (variant b) or without the correction (variant h) it is not, which test_planted_variants shows"""
    k, ru = th.case(c), th.rule(oracle, c)
    loss, kept = th.emulate(oracle, k, k["img"])
    assert not th.breaks(ru, loss, kept), c
    assert not _seam_breaks(ru, loss, kept), c


@pytest.mark.parametrize("tb", ["stanford", "ragged"])
def test_a_fixed_seed_yields_the_lane_clouds(oracle, tb):
    """enough box_room points of which every (point, pose) pair is decisive and no seam pair"""
    ln = th.lanes(oracle, tb)
    print("%s: %d of %d points have only decisive pairs" % (tb, len(ln["xyz"]), ln["pool"]))
    assert len(ln["xyz"]) >= max(th.LANE_SIZES)
    assert len(np.unique(ln["xyz"][:max(th.LANE_SIZES)], axis=0)) == max(th.LANE_SIZES)
    count, m64, m32 = th.lane_means(ln, max(th.LANE_SIZES))
    assert (count > 0).all() and (count < max(th.LANE_SIZES)).any() and np.isfinite(m64).all()


# ==================================================================================================================== the device
@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


_GROUPS = {}


def _groups(ops, tb):
    from parity_helpers import T
    if tb not in _GROUPS:
        _GROUPS[tb] = ops.TrimGroups(T(th.table(tb)))
        assert _GROUPS[tb].ngroups == len(th.classes(th.table(tb))["groups"]), tb
    return _GROUPS[tb]


def _launch(ops, cloud, pano, trans, groups, **kw):
    from parity_helpers import T
    table, count = ops.trim_loss_table(cloud, pano, T(trans), groups, return_count=True, **kw)
    return table.cpu().numpy().reshape(-1), count.cpu().numpy().reshape(-1)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else a, np.asarray(b).view(np.uint32)
                          if np.asarray(b).dtype == np.float32 else b)


def check_pairs(parity, tag, table, count, ru, generic=None):
    """table / count (K R,) of the device against the rule `ru`: count and NaN pattern exactly on the decisive pairs, the loss's median /
    99th percentile / worst relative error at gh.FACTOR x the fp32 model's; the seam pairs against generic(idx) -> (loss, count) of the
    generic forward kernel on the same pairs, with the same bound.  Every figure is printed before the first assert."""
    table = np.asarray(table, np.float64)
    ok, kept = ru["ok"], ru["kept"]
    sel = ok & kept
    s = max(float(np.median(ru["l64"][sel])), 1e-300)
    yard = gh.three_stats(th.errors(ru["l32"], ru["l64"], sel, s))
    dev = gh.three_stats(th.errors(table, ru["l64"], sel, s))
    print("%s: %d pairs, %d border, %d seam, %d kept; loss median / p99 / worst %.3e %.3e %.3e (fp32 model %.3e %.3e %.3e)"
          % ((tag, len(ok), int(ru["border"].sum()), int(ru["seam"].sum()), int(sel.sum())) + dev + yard))
    sidx = np.nonzero(ru["seam_ok"])[0]
    if generic is not None and len(sidx):
        gl, gc = generic(sidx)
        gk = gc == 1
        sdev = gh.three_stats(th.errors(table[sidx], gl, gk, s))
        print("%s: %d seam pairs against the generic kernel: %.3e %.3e %.3e; ends differ at %s" % ((tag, len(sidx)) + sdev + (sidx[count[sidx] != gc][:8],)))
    e = th.errors(table, ru["l64"], sel, s)
    worst = np.nonzero(sel)[0][np.argsort(e)[-3:]] if sel.any() else []
    print("%s: worst pairs %s rho %s" % (tag, list(worst), [float(ru["rho"][i]) for i in worst]))
    bad = np.nonzero(ok & (count != kept))[0]
    assert len(bad) == 0, "%s: count differs from the float64 model's mask at pairs %s" % (tag, bad[:8])
    bad = np.nonzero(ok & (np.isnan(table) != ~kept))[0]
    assert len(bad) == 0, "%s: NaN pattern differs from the model's masked pairs at %s" % (tag, bad[:8])
    assert np.isin(count, (0.0, 1.0)).all()
    for what, a, y in zip(("median", "99th percentile", "worst"), dev, yard):
        parity(tag + ": loss per pair, " + what, a, gh.FACTOR * y, y)
    if generic is not None and len(sidx):
        assert np.array_equal(count[sidx], gc), "%s: seam pairs land on another end than the generic kernel: %s" % (tag, sidx[count[sidx] != gc][:8])
        assert np.array_equal(np.isnan(table[sidx]), ~gk)
        for what, a, y in zip(("median", "99th percentile", "worst"), sdev, yard):
            parity(tag + ": seam pairs vs the generic kernel, " + what, a, gh.FACTOR * y, y)


def _formats(pano):
    return ("u8",) if pano == "lv1024" else ("f32", "f16", "u8")


@gpu
@pytest.mark.parametrize("c", CASES, ids=th.case_id)
def test_one_point_pairs(ops, oracle, parity, c):
    """every (translation, rotation) pair of a one-point case, float4 / fp16-level / RGBA8 texels; the paired RGBA8 layouts bit for bit"""
    from parity_helpers import T
    k = th.case(c)
    groups = _groups(ops, c[2])
    cloud = ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :]))
    tt, rr = th.pairs(k["trans"], k["rot"])
    for fmt in _formats(c[1]):
        pano = ops.Pano(T(k["imgf"] if fmt == "f32" else k["img"]), fmt=fmt)
        table, count = _launch(ops, cloud, pano, k["trans"], groups)

        def generic(idx):
            out = ops.sampling_loss(cloud, pano, T(tt[idx]), T(rr[idx]), with_grad=False).cpu().numpy()
            return out[:, 0].astype(np.float64), out[:, 1]
        check_pairs(parity, "%s %s" % (th.case_id(c), fmt), table, count, th.rule(oracle, c, fmt == "f32"), generic)
        if fmt == "u8":
            for paired in ("u8p", "u8v"):
                tp, cp = _launch(ops, cloud, ops.Pano(T(k["img"]), fmt=paired), k["trans"], groups)
                assert _same_bits(tp, table) and np.array_equal(cp, count), (c, paired)


@gpu
@pytest.mark.parametrize("tb", ["stanford", "ragged"])
@pytest.mark.parametrize("n", th.LANE_SIZES)
def test_every_lane_and_both_halves(ops, oracle, parity, n, tb):
    """clouds of n distinct points of which every pair is decisive: the count of every entry exactly, the entry against the float64 mean of
    the model's kept terms at gh.FACTOR x the error of the float32 model's mean (float32 terms, summed and divided in float32), median /
    99th percentile / worst over the K R entries of a launch.  One point off by a texel moves an entry of these sizes by 1e-4 or more."""
    from parity_helpers import T
    ln = th.lanes(oracle, tb)
    groups = _groups(ops, tb)
    count, m64, m32 = th.lane_means(ln, n)
    yard = gh.three_stats(np.abs(m32 - m64) / m64)
    for sort in (True, False):
        cloud = ops.Cloud(T(ln["xyz"][:n]), T(ln["rgb"][:n]), sort=sort)
        ref = None
        for fmt in ("u8", "u8p", "u8v", "f16"):
            table, cnt = _launch(ops, cloud, ops.Pano(T(ln["img"]), fmt=fmt), th.LANE_TRANS, groups)
            dev = gh.three_stats(np.where(np.isfinite(table), np.abs(table - m64) / m64, np.inf))
            print("n=%d %s sort=%d %s: median / p99 / worst %.3e %.3e %.3e (fp32 model %.3e %.3e %.3e)" % ((n, tb, sort, fmt) + dev + yard))
            assert np.array_equal(cnt, count.astype(np.float32)), (n, tb, sort, fmt, np.nonzero(cnt != count)[0][:8])
            if fmt == "u8":
                ref = table
            elif fmt != "f16":
                assert _same_bits(table, ref), (n, tb, sort, fmt)
            for what, a, y in zip(("median", "99th percentile", "worst"), dev, yard):
                parity("n=%d %s sort=%d %s: entry vs the fp64 mean, %s" % (n, tb, sort, fmt, what), a, gh.FACTOR * y, y)


@gpu
@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("name", ["fractions", "black"])
def test_copies_of_a_point(ops, oracle, name, n):
    """n copies of a probe point (every lane, both halves; 1024: two steps): count n x kept, the loss within n x 2^-24 relative of the
    one-point value (every lane holds the same term; the sums add n same-signed copies of it, fewer than n roundings on any path)"""
    from parity_helpers import T
    c = (name, "probe", "stanford")
    k, ru = th.case(c), th.rule(oracle, c)
    groups = _groups(ops, "stanford")
    pano = ops.Pano(T(k["img"]), fmt="u8")
    one, c1 = _launch(ops, ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :])), pano, k["trans"], groups)
    many, cn = _launch(ops, ops.Cloud(T(np.repeat(k["x"][None, :], n, 0)), T(np.repeat(k["rgb"][None, :], n, 0))), pano, k["trans"], groups)
    assert np.array_equal(cn, n * c1) and np.array_equal(np.isnan(many), np.isnan(one))
    assert np.array_equal(c1[ru["ok"]], ru["kept"][ru["ok"]].astype(np.float32))
    kept = c1 == 1
    rel = np.abs(many[kept].astype(np.float64) - one[kept]) / one[kept]
    print("%s n=%d: worst relative difference %.3e (bound %.3e)" % (name, n, rel.max(), n * U))
    assert (rel <= n * U).all()


@gpu
@pytest.mark.parametrize("images,tb", [(3, "stanford"), (8, "ragged")])
def test_images_and_colour_sets(ops, oracle, parity, images, tb):
    """the `fractions` translations with one panorama and one colour of the point per image, through Cloud.with_color_sets, without and with
    a work list (8 images: the XCD-to-image mapping): every [i, k, r] is the single-image, single-colour launch bit for bit and holds the
    one-point bound against image i's model"""
    import torch
    from parity_helpers import T
    k = th.case(("fractions", "probe", tb))
    groups = _groups(ops, tb)
    rng = np.random.default_rng(images)
    imgs = [th.levels_pano(64, 128, seed=1 + i) for i in range(images)]
    rgbs = [rng.uniform(0.1, 0.9, 3).astype(np.float32) for _ in range(images)]
    X = T(k["x"][None, :])
    for fmt in ("u8", "u8p"):
        panos = [ops.Pano(T(im), fmt=fmt) for im in imgs]
        cloud = ops.Cloud.with_color_sets(X, [T(c[None, :]) for c in rgbs])
        order = ops.TrimOrder(cloud, (64, 128, panos[0].fmt), T(k["trans"]), groups)
        plain = ops.trim_loss_tables(cloud, panos, T(k["trans"]), groups, return_count=True)
        listed = ops.trim_loss_tables(cloud, panos, T(k["trans"]), groups, return_count=True, order=order)
        torch.cuda.synchronize()
        for i in range(images):
            table, count = _launch(ops, ops.Cloud(X, T(rgbs[i][None, :])), panos[i], k["trans"], groups)
            for tabs, how in ((plain, "sets"), (listed, "sets + list")):
                assert _same_bits(tabs[0][i].cpu().numpy().reshape(-1), table) and np.array_equal(tabs[1][i].cpu().numpy().reshape(-1), count), (fmt, i, how)
            if fmt == "u8":
                check_pairs(parity, "fractions %s image %d of %d" % (tb, i, images), table, count, th.rule_for(oracle, k, imgs[i], rgbs[i]))
