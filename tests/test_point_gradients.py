"""The loss kernel's gradient, point by point against a float64 model (tests/grad_helpers.py).

The 8 accumulators of pcl_loss_kernel are linear in the points, so one point per pose row gives every point's own
[l, 1, grad_t, grad_ypr]: through a one-hot `visible` row (B = n copies of a pose: the VIS = 1 gradient instances, every lane, both packed
halves, several steps and a ragged last one) and through clouds of one point under probe poses that put it where kernels go wrong (the
VIS = 0 instances a refinement runs).  The CPU part ties the model to the oracle's loss, holds the share of border pairs under its cap by
the model alone and shows that each planted mistake of the model breaks the bound the device is held to."""
import ctypes

import numpy as np
import pytest

import grad_helpers as gh

gpu = pytest.mark.gpu

FMTS = ("f16", "u8", "f32", "float")        # "float": the case's float image that is not k/255, float4 texels
U = 2.0 ** -24                               # unit roundoff of fp32

# which case catches which planted variant (asserted below); ("case", name, pose) or ("probe", name)
CATCHERS = {
    "clip_passes": [("case", "G2", 0), ("probe", "seam"), ("probe", "poles")],
    "no_eps": [("probe", "rho"), ("probe", "axis")],
    "edge_clamp": [("case", "tiny", 0), ("probe", "border16")],
    "align_corners": [("case", "G2", 0), ("case", "fine", 1), ("probe", "fractions")],
    "pitch_roll": [("case", "odd", 1), ("case", "tall", 0), ("probe", "border300")],
    "skip_black": [("case", "G2", 1), ("probe", "black")],
    "d0_nan": [("probe", "const")],
}


# ================================================================================================== the model and the rule (CPU)
@pytest.mark.parametrize("name", list(gh.CASES))
def test_the_model_is_the_oracle(oracle, name):
    """per point the model equals the rows of oracle.sampling_loss(..., visible=identity) in float64: mask and NaN pattern exactly, loss and
    gradient to float64 rounding (1e-12 of max(the row's size, the case's median row size): the two sum the same products in another order)"""
    xyz, rgb, img, imgf, trans, rot = gh.scene(oracle, name)
    for flt in (False, True):
        for b in range(gh.N_POSES):
            m = gh.case_model(oracle, name, b, flt)
            loss, count, grad = gh.oracle_rows(oracle, xyz, rgb, imgf if flt else img, trans[b], rot[b])
            assert np.array_equal(count, m["kept"].astype(np.int64)), (name, flt, b)
            assert np.array_equal(np.isnan(grad), np.isnan(m["grad"])) and np.array_equal(np.isnan(loss), ~m["kept"])
            k = m["kept"]
            assert k.sum() > len(k) // 2
            assert np.abs(loss[k] - m["loss"][k]).max() <= 1e-12 * np.abs(loss[k]).max(), (name, flt, b)
            worst = gh.three_stats(gh.point_errors(m["grad"], grad, k))[2]
            assert worst <= 1e-12, (name, flt, b, worst)


def test_the_numpy_taps_are_the_oracle(oracle):
    """taps() (used by two planted variants) without a mode is the oracle's sample and sample backward, zero border and clip included"""
    xyz, rgb, img, _, trans, rot = gh.scene(oracle, "tiny")
    m = gh.case_model(oracle, "tiny", 0)
    coord = np.stack([m["gx"], m["gy"]], 1)
    im = img.astype(np.float64)
    c, dcdx, dcdy = gh.taps(im, coord)
    assert np.abs(c - oracle.sample_from_img(im, coord, np.float64)).max() <= 1e-15
    u = np.random.default_rng(0).normal(size=c.shape)
    gc = oracle.sample_from_img_backward(im, coord, u, np.float64, want_img=False)[0]
    mine = np.stack([np.where(m["in_x"], (u * dcdx).sum(1) * 9 / 2, 0), np.where(m["in_y"], (u * dcdy).sum(1) * 7 / 2, 0)], 1)
    assert np.abs(mine - gc).max() <= 1e-13 * np.abs(gc).max()
    assert (~m["in_x"]).any() and (m["ix"] < 0).any() and (m["iy"] < 0).any()                   # clipped points and zero-border taps took part


@pytest.mark.parametrize("name", list(gh.CASES))
def test_border_pairs_stay_under_the_cap(oracle, name):
    """by the model alone: at most 1 % of a case's pairs are border pairs, and delta is what fp32 pixel coordinates of that size give"""
    n, H, W, _ = gh.CASES[name]
    dropped = 0
    for b in range(gh.N_POSES):
        m64, m32, ok, delta, gap = gh.case_rule(oracle, name, b)
        print("%s pose %d: gap %.3e px, delta %.3e px, dropped %d of %d, kept %d, masked %d" % (name, b, gap, delta, (~ok).sum(), n, m64["kept"].sum(),
                                                                                          (~m64["kept"]).sum()))
        assert 0 < delta <= 3 * 4 * max(H, W) * 2.0 ** -23, (name, b, delta)                   # gap: a few ulps of the largest pixel coordinate
        dropped += int((~ok).sum())
    assert dropped <= gh.BORDER_CAP * n * gh.N_POSES, (name, dropped)
    if name != "tiny":
        assert (~gh.case_model(oracle, name, 0)["kept"]).any()                                 # masked points exist


@pytest.mark.parametrize("name", gh.PROBES)
def test_no_probe_is_a_border_pair(oracle, name):
    """the probes are aimed away from every boundary: none is dropped, and each class holds what it is for"""
    k = gh.probe(oracle, name)
    m = k["m64"]
    assert k["ok"].all(), (name, np.nonzero(~k["ok"])[0])
    assert len(k["trans"]) % 2 == 1 and len(k["trans"]) >= 71
    fx, fy = m["ix"] - np.floor(m["ix"]), m["iy"] - np.floor(m["iy"])
    inx, iny = m["in_x"], m["in_y"]
    assert np.minimum(fx, 1 - fx)[inx].min() >= 0.049 and (not iny.any() or np.minimum(fy, 1 - fy)[iny].min() >= 0.049)
    x0, y0 = np.floor(np.clip(m["ix"], -1, m["W"])), np.floor(np.clip(m["iy"], -1, m["H"]))
    if name == "seam":
        assert inx.any() and (~inx).any() and (m["gx"] > 0.9999).any() and (m["gx"] < -0.9999).any()
    if name in ("poles", "axis"):
        assert iny.any() and (~iny & (m["gy"] > 0)).any() and (~iny & (m["gy"] < 0)).any()
    if name == "border16":
        outx, outy = inx & ((x0 < 0) | (x0 + 1 >= m["W"])), iny & ((y0 < 0) | (y0 + 1 >= m["H"]))
        assert (outx & ~outy).any() and (outy & ~outx).any() and (outx & outy).any()
    if name == "black":
        assert (~m["kept"]).sum() >= 40 and m["kept"].sum() >= 120
    if name == "const":
        assert (m["loss"] <= 4e-16).all() and (m["loss"] == 0).any() and (m["grad"] == 0).all()      # (l = 0 up to the weights' rounding)
    if name == "rho":
        r = np.sqrt((m["p"] ** 2).sum(1))
        assert r.min() < 1.1e-3 and r.max() > 0.9e3
    if name == "axis":
        s = np.hypot(m["p"][:, 0], m["p"][:, 1]) / np.sqrt((m["p"] ** 2).sum(1))
        assert s.min() < 1.1e-3 and 0.09 < s.max() < 0.11


def _variant_breaks(oracle, variant, where):
    """does the planted variant break the device bound (gh.FACTOR x the fp32 model's statistics) on the decisive pairs of `where`?"""
    if where[0] == "case":
        m64, m32, ok, _, _ = gh.case_rule(oracle, where[1], where[2])
        mv = gh.case_model(oracle, where[1], where[2], variant=variant)
    else:
        k = gh.probe(oracle, where[1])
        m64, m32, ok = k["m64"], k["m32"], k["ok"]
        mv = gh.model(oracle, k["x"][None, :], k["rgb"][None, :], k["img"], k["trans"], k["rot"], np.float64, variant)
    if not np.array_equal(mv["kept"][ok], m64["kept"][ok]):
        return True
    sel = ok & m64["kept"]
    yard = gh.three_stats(gh.point_errors(m32["grad"], m64["grad"], sel))
    got = gh.three_stats(gh.point_errors(mv["grad"], m64["grad"], sel))
    print("%s on %s: variant %.3e %.3e %.3e, fp32 model %.3e %.3e %.3e" % ((variant, where) + got + yard))
    return gh.exceeds(got, yard)


@pytest.mark.parametrize("variant", list(gh.VARIANTS))
def test_planted_variants_break_the_bound(oracle, variant):
    """each planted mistake of the model is further from the model than the device may be (its median, 99th percentile or worst e_i over the decisive pairs above
    gh.FACTOR x the fp32 model's: what check_pairs asserts of the device), on every case named for it in CATCHERS"""
    for where in CATCHERS[variant]:
        assert _variant_breaks(oracle, variant, where), (gh.VARIANTS[variant], where)


# ==================================================================================================================== the device
@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def check_pairs(parity, tag, out, m64, m32, ok):
    """out (m,8) of the device against the model on the decisive pairs `ok`: count and NaN pattern exactly, the loss as the residual test
    bounds it, the gradient's median / 99th percentile / worst e_i at gh.FACTOR x the fp32 model's.  Every figure is printed before the
    first assert.  -> (the device's statistics, the yardsticks)"""
    out = np.asarray(out, np.float64)
    kept = m64["kept"]
    sel = ok & kept
    lgap = float(np.abs(m32["loss"].astype(np.float64) - m64["loss"])[sel].max()) if sel.any() else 0.0
    lerr = float(np.abs(out[:, 0] - m64["loss"])[sel].max()) if sel.any() else 0.0
    yard = gh.three_stats(gh.point_errors(m32["grad"], m64["grad"], sel))
    dev = gh.three_stats(gh.point_errors(out[:, 2:8], m64["grad"], sel))
    print("%s: %d pairs, %d border, %d kept; loss %.3e (fp32 model %.3e); gradient median / p99 / worst %.3e %.3e %.3e (fp32 model %.3e %.3e %.3e)"
          % ((tag, len(ok), int((~ok).sum()), int(sel.sum()), lerr, lgap) + dev + yard))
    bad = np.nonzero(ok & (out[:, 1] != kept))[0]
    assert len(bad) == 0, "%s: count differs from the float64 model's mask at pairs %s" % (tag, bad[:8])
    nan = np.isnan(out[:, [0, 2, 3, 4, 5, 6, 7]])
    bad = np.nonzero(ok & (nan != ~kept[:, None]).any(1))[0]
    assert len(bad) == 0, "%s: NaN pattern differs from the model's masked rows at pairs %s" % (tag, bad[:8])
    parity(tag + ": loss per point vs fp64", lerr, gh.FACTOR * lgap, lgap)
    for what, a, y in zip(("median", "99th percentile", "worst"), dev, yard):
        parity(tag + ": gradient per point, " + what, a, gh.FACTOR * y, y)
    return dev, yard


_CLOUDS, _PANOS, _EYES = {}, {}, {}


def _device_case(ops, oracle, name, fmt, sort):
    from parity_helpers import T
    xyz, rgb, img, imgf, trans, rot = gh.scene(oracle, name)
    if (name, sort) not in _CLOUDS:
        _CLOUDS[name, sort] = ops.Cloud(T(xyz), T(rgb), sort=sort)
    if (name, fmt) not in _PANOS:
        _PANOS.clear()                                       # (one panorama at a time: the 1024 x 2048 float4 one is 34 MB)
        _PANOS[name, fmt] = ops.Pano(T(imgf if fmt == "float" else img), fmt="f32" if fmt == "float" else fmt)
    n = len(xyz)
    if n not in _EYES:
        import torch
        _EYES[n] = torch.eye(n, dtype=torch.uint8, device="cuda")
    return _CLOUDS[name, sort], _PANOS[name, fmt], _EYES[n]


def one_hot_rows(ops, cloud, pano, t, ypr, eye):
    """(n,8) in the caller's point order: row i is point i's own [l, 1, grad_t, grad_ypr] (`visible` is in packed order)"""
    from parity_helpers import T
    n = cloud.n
    out = ops.sampling_loss(cloud, pano, T(np.repeat(t.reshape(1, 3), n, 0)), T(np.repeat(ypr.reshape(1, 3), n, 0)), visible=eye).cpu().numpy()
    if cloud.order is not None:
        back = np.empty_like(out)
        back[cloud.order.cpu().numpy()] = out
        out = back
    return out


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(gh.CASES))
def test_one_hot_rows(ops, oracle, parity, name, fmt):
    """B = n copies of a start pose with an identity mask, sorted and unsorted pack, two start poses: every decisive point's own term"""
    n = gh.CASES[name][0]
    G = ctypes.c_int(0)
    assert ops._lib.load().pcl_gd_plan(n, n, None, ctypes.byref(G), None) == 0
    assert G.value == (2 if n % 2 == 0 else 1), (name, G.value)
    trans, rot = gh.scene(oracle, name)[4:6]
    for sort in (True, False):
        cloud, pano, eye = _device_case(ops, oracle, name, fmt, sort)
        assert (cloud.order is not None) == sort
        for b in range(gh.N_POSES):
            m64, m32, ok, _, _ = gh.case_rule(oracle, name, b, fmt == "float")
            out = one_hot_rows(ops, cloud, pano, trans[b], rot[b], eye)
            check_pairs(parity, "%s %s sort=%d pose %d" % (name, fmt, sort, b), out, m64, m32, ok)


def _probe_device(ops, k, fmt, B):
    from parity_helpers import T
    cloud = ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :]))
    return ops.sampling_loss(cloud, ops.Pano(T(k["img"]), fmt=fmt), T(k["trans"][:B]), T(k["rot"][:B])).cpu().numpy()


def _head(m, B):
    return {key: (v[:B] if isinstance(v, np.ndarray) else v) for key, v in m.items()}


@gpu
@pytest.mark.parametrize("fmt", FMTS[:3])
@pytest.mark.parametrize("name", gh.PROBES)
def test_probe_poses(ops, oracle, parity, name, fmt):
    """a cloud of one point under the poses of a probe class, B odd (one pose per block) and B - 1 (two): the same bound per class; the part
    of the gradient that belongs to a clipped coordinate is exactly 0 in the model and 0 within the bound on the device"""
    k = gh.probe(oracle, name)
    full = len(k["trans"])
    for B in (full, full - 1):
        m64, m32, ok = _head(k["m64"], B), _head(k["m32"], B), k["ok"][:B]
        out = _probe_device(ops, k, fmt, B)
        dev, yard = check_pairs(parity, "%s %s B=%d" % (name, fmt, B), out, m64, m32, ok)
        sel = ok & m64["kept"]
        if name == "const":
            assert (out[:, 2:8] == 0).all() and np.isfinite(out).all(), (name, fmt, out[:4])
        # clipped coordinates: dl/dgx (dl/dgy) is exactly 0 in the model; the device's camera-frame g = -R grad_t has no such part
        assert (m64["gc"][~m64["in_x"], 0] == 0).all() and (m64["gc"][~m64["in_y"], 1] == 0).all()
        R = gh.rotations(oracle, k["rot"][:B], np.float64)[0]
        with np.errstate(invalid="ignore"):
            part_phi, part_th = gh.angle_parts(m64, -gh._apply(R, out[:, 2:5].astype(np.float64)))
        rn = np.abs(m64["grad"]).max(1)
        scale = np.maximum(rn, max(float(np.median(rn[sel])), 1e-300) if sel.any() else 1.0)
        for what, part, clipped in (("phi", part_phi, sel & ~m64["in_x"]), ("theta", part_th, sel & ~m64["in_y"])):
            if clipped.any():
                parity("%s %s B=%d: clipped %s part of the gradient" % (name, fmt, B, what), float((part / scale)[clipped].max()), gh.FACTOR * yard[2],
                       yard[2])


@gpu
@pytest.mark.parametrize("n", [512, 1024])
@pytest.mark.parametrize("name", ["fractions", "black"])
def test_copies_of_a_point_sum_to_the_point(ops, oracle, name, n):
    """the probe's point copied n times (every lane, both packed halves; 1024: two steps): count n, loss and gradient those of the
    single-point launch.

    The bound counts roundings and measures nothing.  Every lane of every wave holds the same term v_k in accumulator k (one step per
    block: acc = 0 + v_k, exact; the same instruction stream on the same inputs as the single-point launch, whose other lanes add zeros:
    its sums are v_k exactly).  pcl_loss.hip then adds on the longest path: the two packed halves (1), four DPP steps inside a row of 16
    lanes (4), the four row sums pairwise (2), the four waves' sums one after the other (3): 10 fp32 additions of same-signed multiples
    of v_k, each within u = 2^-24: |S_k - n v_k| <= ((1 + u)^10 - 1) n |v_k|.  The chunks' partials are added in double and the chain rule
    (pcl_gd_device.h) runs in double, one rounding to fp32 per output and launch: grad_t = -R^T sum g / M with |R_jk| <= 1, so
    |d grad_t_k| <= 10 u ||g||_1 + 2 u |grad_t_k|; the angles are combinations of the torque sum with coefficients of size <= 1:
    |d grad_ypr_k| <= 10 u ||p x g||_1 + 2 u |grad_ypr_k|; the loss is (float) S_0 / (float) M: 10 u l + three roundings per launch.
    g and p x g are the model's (the device's are within 1e-3 of them, asserted by test_probe_poses; 1.01 covers that)."""
    from parity_helpers import T
    k = gh.probe(oracle, name)
    B = len(k["trans"]) - 1
    m64 = _head(k["m64"], B)
    pano = ops.Pano(T(k["img"]), fmt="f16")
    one = ops.sampling_loss(ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :])), pano, T(k["trans"][:B]), T(k["rot"][:B])).cpu().numpy().astype(np.float64)
    cloud = ops.Cloud(T(np.repeat(k["x"][None, :], n, 0)), T(np.repeat(k["rgb"][None, :], n, 0)))
    many = ops.sampling_loss(cloud, pano, T(k["trans"][:B]), T(k["rot"][:B])).cpu().numpy().astype(np.float64)
    kept = m64["kept"]
    assert np.array_equal(one[:, 1], kept.astype(np.float64)) and np.array_equal(many[:, 1], n * kept.astype(np.float64))
    assert np.array_equal(np.isnan(many), np.isnan(one)) and np.array_equal(np.isnan(many[:, 0]), ~kept)
    adds = (1 + U) ** 10 - 1
    g1, tau1 = 1.01 * np.abs(m64["g"]).sum(1)[kept, None], 1.01 * np.abs(m64["tau"]).sum(1)[kept, None]
    a, b = one[kept], many[kept]
    assert (np.abs(b[:, 0] - a[:, 0]) <= (adds + 6 * U) * np.abs(a[:, 0])).all()
    assert (np.abs(b[:, 2:5] - a[:, 2:5]) <= adds * g1 + 2 * U * np.abs(a[:, 2:5])).all(), np.abs(b[:, 2:5] - a[:, 2:5]).max()
    assert (np.abs(b[:, 5:8] - a[:, 5:8]) <= adds * tau1 + 2 * U * np.abs(a[:, 5:8])).all(), np.abs(b[:, 5:8] - a[:, 5:8]).max()
