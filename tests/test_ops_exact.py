"""The stand-alone ops (csrc/pcl_ops.hip) element by element against the plain numpy models of tests/ops_models.py.

The rule: every op is compared with a float64 or integer model of the same operation on seeded inputs, at the shapes where a kernel goes
wrong (one row or column, odd sizes, 255 / 256 / 257 points, a second trip of a grid-stride loop), and whatever is exact is compared with
array_equal.

make_pano / scatter_min_depth: the inputs are constructed so that fp32 cannot move a point across a pixel edge (condition 1: the fp32 and
  fp64 oracles and the model agree on every pixel, generated points sit at fractions in [0.2, 0.8]) and a contracted x*x + y*y + z*z cannot
  reorder two depths (condition 2: depths a relative 1e-3 apart, or rows equal in |x|, |y|, |z|).  Winners, arg and images are then EQUAL;
  zmin is within the documented one ulp of contraction (rtol 2.5e-7) of the float64 norm.
cloud2idx: 5e-7 absolute against float64 (ocml atan2f: about two ulp of O(1) coordinates, the bound of the golden test), exact values on
  the axes and the seam.  Its backward: twice the fp32 model's own distance from float64 plus 1e-6, relative to max(|ref|, 1), on every
  point INCLUDING the axis points (rho = 0), where the norm's subgradient is 0: finite, and exactly zero x and y from that branch.
  (The fp32 form of this kernel missed the bound: 2.21e-5 against 2.06e-5, at a point 4e-4 from the camera whose phi and rho terms are 300
  times their sum; the contracted fp32 formulas evaluated in numpy give the same 2.2056513e-5, so it was fp32's own loss there, twice the
  uncontracted model's.  The kernel now evaluates in fp64 and rounds once.)
transform_cloud: per component |out - R (x - t)| <= 5e-7 (|qx| + |qy| + |qz|).  Derivation: the device's R is within 2e-7 of the float64 R
  (test_rot_from_ypr); q = x - t carries one rounding, the product and the two fmas three more, each 2^-24 = 6e-8 of a partial sum that
  is at most |q|_1 (|R_ij| <= 1): 2e-7 + 4 * 6e-8 < 5e-7.
quantile_box: order statistics, exact, a second trip of the histogram's grid-stride loop included; q = 0 and q = 1 raise.
sample_from_img: clip to +-0.99 in fp32, then bilinear taps in float64.  Forward: twice the fp32 model's own gap to float64 plus 1e-7, per
  case; u8 and f16 texels bit-equal.  Backward: grad_coord at twice the fp32 model's gap plus 1e-5 and EXACTLY 0 outside the clip;
  grad_img, accumulated by float atomics in no fixed order, inside om.atomic_sum_bound per texel channel: the fp32 summation bound
  (m + 3) 2^-24 sum|c| (m contributions: m - 1 additions, and three roundings in each contribution's weight and product) plus the rounding
  of the fp32 weights themselves, 2.5 (W + H) 2^-24 sum|gout| (derived there); a texel nothing reaches stays exactly 0, so nothing comes
  from the zero border; row and column sums of the weights alone likewise.  4096 points on 2 x 3 texels are held to the summation bound
  alone, sums from the float64 model.  On dyadic inputs every sum is exact and grad_img EQUALS the model.
  A coordinate whose ix or iy lies within 1e-4 of an integer on a size that is no power of two is not decidable (the fp32 floor may fall
  either way, and the gradient of a bilinear image jumps there): it is left out of the zero-pattern and grad_coord comparisons, never
  given a tolerance; on power-of-two sizes pixel centres are exact in every arithmetic and stay in.
The CPU part asserts the two conditions, holds the fp32 oracle to the same comparison, and plants plausible kernel mistakes into the models:
each must break the comparison the device is held to."""
import functools

import numpy as np
import pytest

import ops_models as om

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64

# (H, W, n, duplicated rows): every resolution from one pixel up; 255 / 256 / 257 points around the block size; H W = 63 and 2112 are no
# multiple of 256; 70 points on the 2 x 4 centre pixels of 3 x 5: several per pixel at distinct depths; 100 duplicated rows on 16 x 32;
# two sparse clouds, where splats stand alone or overlap in part and the EARLY passes stay visible (a dense cloud shows the late ones only),
# and "pairs": for every two passes a pixel that just these two reach (om.pass_pairs_case)
PANO_CASES = [(1, 1, 12, 0), (1, 2, 12, 0), (2, 1, 12, 0), (2, 2, 14, 0), (3, 5, 70, 0), (7, 9, 255, 0), (7, 9, 256, 0), (7, 9, 257, 6),
              (16, 32, 1200, 100), (16, 32, 60, 4), (33, 64, 300, 0), (33, 64, 81, "pairs"), (33, 64, 3000, 0)]
CPU_ONLY_CASES = [(64, 128, 9000, 50)]


def _id(c):
    return "%dx%d-n%d" % c[:3]


@functools.lru_cache(maxsize=None)
def pano_case(c):
    H, W, n, dup = c
    k = om.pass_pairs_case(H, W, seed=n) if dup == "pairs" else om.pano_case(H, W, n, seed=1000 * H + W + n, dup=dup)
    assert len(k["xyz"]) == n
    k["row"], k["col"], k["frow"], k["fcol"] = om.pano_pixels(k["xyz"], H, W)
    k["winner"], k["pass"] = om.make_pano_winners(k["xyz"], H, W, k["row"], k["col"])
    k["image"] = om.pano_image(k["winner"], k["rgb"], H, W)
    k["zmin"], k["arg"] = om.scatter_min(k["xyz"], H, W, k["row"], k["col"])
    return k


SINGLE_RES = [(1, 1), (2, 2), (7, 9)]


def single_cases():
    """every special point alone (n = 1), at three resolutions"""
    for H, W in SINGLE_RES:
        for p in om.special_points(H, W, [1.0, 1.0, 2.0, 2.0, 2.0, 2.0]):
            yield H, W, p.reshape(1, 3).copy(), np.array([[0.25, 0.5, 1.0]], F32)


# ===================================================================================================== conditions 1 and 2 (CPU)
def test_pass_order_is_the_oracles(oracle):
    assert om.PANO_PASSES == oracle.PANO_PASSES


@pytest.mark.parametrize("c", PANO_CASES + CPU_ONLY_CASES, ids=_id)
def test_constructed_points_are_decidable(oracle, c):
    """condition 1: the fp32 oracle, the fp64 oracle and the model agree on every point's pixel, and every generated point sits at a
    fraction in [0.2, 0.8] of it; condition 2: the depths are separated; the special points land where they are meant to"""
    k = pano_case(c)
    H, W, xyz = k["H"], k["W"], k["xyz"]
    r32, c32 = oracle.pano_pixels(xyz, (H, W), np.float32)
    r64, c64 = oracle.pano_pixels(xyz, (H, W), np.float64)
    assert np.array_equal(r32, r64) and np.array_equal(c32, c64)
    assert np.array_equal(r64, k["row"]) and np.array_equal(c64, k["col"])
    g = k["generated"]
    if H > 1:
        assert 0.2 <= k["frow"][g].min() and k["frow"][g].max() <= 0.8
    if W > 1:
        assert 0.2 <= k["fcol"][g].min() and k["fcol"][g].max() <= 0.8
    assert om.depth_separation(xyz) >= om.DEPTH_GAP
    # the special points: axis, seam, origin
    on_axis = (xyz[:, 0] == 0) & (xyz[:, 1] == 0)
    assert (k["row"][on_axis & (xyz[:, 2] >= 0)] == 0).all() and (k["row"][on_axis & (xyz[:, 2] < 0)] == H - 1).all()
    assert (on_axis & (xyz[:, 2] > 0)).sum() == 1 and (on_axis & (xyz[:, 2] < 0)).sum() == 1 and (on_axis & (xyz[:, 2] == 0)).sum() == 1
    seam = (xyz[:, 0] == -1) & (xyz[:, 1] == 0) & (xyz[:, 2] == 0)
    neg = np.signbit(xyz[:, 1])
    assert (seam & neg).sum() == 1 and (seam & ~neg).sum() == 1
    assert (k["col"][seam & neg] == W - 1).all() and (k["col"][seam & ~neg] == 0).all()
    # every centre pixel is some point's, the clamped rows and columns among them
    if c[3] == "pairs":
        return
    assert len(np.unique(k["row"][g] * W + k["col"][g])) == min(int(g.sum()) - c[3], max(H - 1, 1) * max(W - 1, 1))
    if c[3]:
        # duplicated rows (the seam points differ in the sign of a zero only and do not count): test_planted_tie_rule_... shows they decide
        _, inv, cnt = np.unique(xyz, axis=0, return_inverse=True, return_counts=True)
        assert ((cnt[inv.reshape(-1)] > 1) & ~seam).sum() == 2 * c[3]


def test_single_special_points_are_decidable(oracle):
    for H, W, xyz, _ in single_cases():
        r32, c32 = oracle.pano_pixels(xyz, (H, W), np.float32)
        r64, c64 = oracle.pano_pixels(xyz, (H, W), np.float64)
        row, col, _, _ = om.pano_pixels(xyz, H, W)
        assert r32[0] == r64[0] == row[0] and c32[0] == c64[0] == col[0], (H, W, xyz)


@pytest.mark.parametrize("c", PANO_CASES, ids=_id)
def test_fp32_oracle_passes_the_comparison(oracle, parity, c):
    """the fp32 restatement of the reference meets the rule the device is held to: equal winners, image, arg; zmin inside one ulp"""
    k = pano_case(c)
    H, W = k["H"], k["W"]
    img, owner, _ = oracle.make_pano(k["xyz"], k["rgb"], (H, W), np.float32, return_aux=True)
    assert np.array_equal(owner.reshape(-1), k["winner"]) and np.array_equal(img, k["image"])
    assert np.array_equal(om.winners_from_image(img, k["rgb"]), k["winner"])
    zmin, arg = oracle.scatter_min_depth(k["xyz"], (H, W), np.float32)
    assert np.array_equal(arg, k["arg"]) and (zmin[k["zmin"] == 0] == 0).all()
    hit = k["zmin"] > 0
    err = (np.abs(zmin[hit] - k["zmin"][hit]) / k["zmin"][hit]).max() if hit.any() else 0.0
    parity("fp32 oracle scatter_min_depth %s: zmin vs sqrt of the float64 norm (rel)" % _id(c), err, 2.5e-7)
    assert (zmin[arg == len(k["xyz"])] == 0).all()


# ===================================================================================================== planted mistakes (CPU)
def _differs_somewhere(cases, **planted):
    hit = []
    for c in cases:
        k = pano_case(c)
        w, _ = om.make_pano_winners(k["xyz"], k["H"], k["W"], k["row"], k["col"], **planted)
        if not np.array_equal(om.pano_image(w, k["rgb"], k["H"], k["W"]), k["image"]):
            hit.append(c)
    return hit


def test_planted_pass_order_breaks_the_comparison():
    for a in range(9):
        for b in range(a):
            passes = list(om.PANO_PASSES)
            passes[a], passes[b] = passes[b], passes[a]
            assert _differs_somewhere(PANO_CASES[3:], passes=passes), (a, b)
    # every pass is some pixel's last one in the cases themselves
    assert {int(p) for c in PANO_CASES for p in pano_case(c)["pass"]} == set(range(-1, 9))          # (-1: pixels nothing reaches)


def test_planted_wrap_at_column_0_breaks_the_comparison():
    """(a dense cloud hides it: what wraps to the last column is overwritten by that column's own later passes)"""
    assert len(_differs_somewhere(PANO_CASES[4:], wrap_col0=True)) >= 2


def test_planted_tie_rule_breaks_the_comparison():
    with_dup = [c for c in PANO_CASES if c[3] not in (0, "pairs")]
    assert len(with_dup) >= 3 and _differs_somewhere(with_dup, tie_smallest=True) == with_dup


def test_planted_scatter_tie_rule_breaks_the_comparison():
    """the z-buffer's tie goes to the SMALLEST index: the largest is a different arg on every case with duplicated rows"""
    for c in (c for c in PANO_CASES if c[3] not in (0, "pairs")):
        k = pano_case(c)
        n = len(k["xyz"])
        _, arg = om.scatter_min(k["xyz"][::-1], k["H"], k["W"], k["row"][::-1], k["col"][::-1])          # smallest reversed = largest
        arg = np.where(arg == n, n, n - 1 - arg)
        assert not np.array_equal(arg, k["arg"])


# ===================================================================================================== sample_from_img inputs
SAMPLE_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 3), (7, 9), (16, 32)]


def _pow2(v):
    return v & (v - 1) == 0


@functools.lru_cache(maxsize=None)
def sample_case(H, W):
    """257 seeded coordinates: the clip's edges and both fp32 neighbours of each, +-1, +-5, +-inf (alone in x, alone in y, in both), pixel
    centres, texel edges, random ones in [-1.2, 1.2]; a k/255 image with black texels and one that is not k/255; a gradient"""
    rng = np.random.default_rng(77 * H + W)
    lim = om.LIM32
    edge = [lim, -lim, np.nextafter(lim, F32(2)), np.nextafter(lim, F32(0)), np.nextafter(-lim, F32(-2)), np.nextafter(-lim, F32(0)),
            F32(1), F32(-1), F32(5), F32(-5), F32(np.inf), F32(-np.inf)]
    co = []
    for v in edge:
        co += [(v, F32(rng.uniform(-0.9, 0.9))), (F32(rng.uniform(-0.9, 0.9)), v), (v, v)]
    ys, xs = np.mgrid[0:H, 0:W]
    pick = rng.permutation(H * W)[:40]
    co += [(F32((2 * x + 1) / W - 1), F32((2 * y + 1) / H - 1)) for y, x in zip(ys.reshape(-1)[pick], xs.reshape(-1)[pick])]      # pixel centres
    ey, ex = np.mgrid[0:H + 1, 0:W + 1]
    pick = rng.permutation((H + 1) * (W + 1))[:40]
    co += [(F32(2 * x / W - 1), F32(2 * y / H - 1)) for y, x in zip(ey.reshape(-1)[pick], ex.reshape(-1)[pick])]                  # texel edges
    coord = np.array(co, F32)
    n_special = len(coord)
    coord = np.concatenate([coord, rng.uniform(-1.2, 1.2, (257 - len(coord), 2)).astype(F32)])
    assert coord.shape == (257, 2) and not np.isnan(coord).any()
    levels = rng.integers(1, 256, (H, W, 3))
    if H * W > 2:
        levels[rng.uniform(size=(H, W)) < 0.3] = 0
        levels[-1, -1] = 255
    imgk = om.levels_image(levels)
    imgs = (imgk * F32(0.93)).astype(F32)
    gout = rng.normal(size=(257, 3)).astype(F32)
    t = om.sample_taps(coord, H, W)
    near = np.minimum(np.abs(t["ix"] - np.rint(t["ix"])), np.abs(t["iy"] - np.rint(t["iy"]))) < 1e-4
    decidable = ~near | (_pow2(H) and _pow2(W))
    return dict(coord=coord, n_special=n_special, levels=levels, imgk=imgk, imgs=imgs, gout=gout, decidable=decidable, H=H, W=W)


def test_sample_cases_hold_what_they_are_for():
    lim = om.LIM32
    for H, W in SAMPLE_SHAPES:
        k = sample_case(H, W)
        c, t = k["coord"], om.sample_taps(k["coord"], H, W)
        assert (c == lim).any() and (c == -lim).any() and np.isinf(c).any()
        assert (~t["inr"]).any(1).sum() >= 30
        assert (~t["inb"]).any(1).sum() >= 10                                   # footprints that reach into the zero border
        assert k["decidable"].mean() > 0.8
        if _pow2(H) and _pow2(W):
            assert k["decidable"].all() and ((t["wx1"] == 0) & (t["wy1"] == 0)).sum() >= min(H * W, 40)       # exact pixel centres
        if H * W >= 63:
            out = om.sample_from_img(k["imgk"], c)
            assert ((out == 0).all(1) & k["decidable"]).any() and (k["levels"] == 0).any()


def test_planted_sampling_mistakes_break_the_comparison(parity):
    """a border tap that is not dropped, a clip that passes the gradient outside +-0.99: both leave the bound the device is held to"""
    for H, W in SAMPLE_SHAPES:
        k = sample_case(H, W)
        m64 = om.sample_from_img_backward(k["imgs"], k["coord"], k["gout"])
        m32 = om.sample_from_img_backward(k["imgs"], k["coord"], k["gout"], F32)
        parity("fp32 model %dx%d: grad_img vs float64 / atomic-sum bound (a sequential fp32 sum sits well inside)" % (H, W),
               _ratio(m32["grad_img"], m64["grad_img"], m64["bound"]), 0.5)
        if H * W > 1:                                   # (one texel: every address folds onto it, the sum cannot tell)
            bad = om.sample_from_img_backward(k["imgs"], k["coord"], k["gout"], keep_border=True)
            assert (np.abs(bad["grad_img"] - m64["grad_img"]) > 100 * m64["bound"]).any()
        bad = om.sample_from_img_backward(k["imgs"], k["coord"], k["gout"], pass_clip=True)
        inr = om.sample_taps(k["coord"], H, W)["inr"]
        assert (bad["grad_coord"][~inr] != 0).any() and (m64["grad_coord"][~inr] == 0).all()


# ===================================================================================================== the device
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


def _check_pano(ops, parity, xyz, rgb, H, W, tag):
    row, col, _, _ = om.pano_pixels(xyz, H, W)
    winner, _ = om.make_pano_winners(xyz, H, W, row, col)
    img = ops.make_pano(T(xyz), T(rgb), (H, W)).cpu().numpy()
    got = om.winners_from_image(img, rgb)
    assert np.array_equal(got, winner), (tag, np.nonzero(got != winner)[0][:8], got[got != winner][:8], winner[got != winner][:8])
    assert np.array_equal(img, om.pano_image(winner, rgb, H, W)), tag
    zmin, arg = ops.scatter_min_depth(T(xyz), (H, W))
    zmin, arg = zmin.cpu().numpy(), arg.cpu().numpy()
    zref, aref = om.scatter_min(xyz, H, W, row, col)
    assert np.array_equal(arg, aref), (tag, np.nonzero(arg != aref)[0][:8])
    assert (zmin[zref == 0] == 0).all()
    hit = zref > 0
    return float((np.abs(zmin[hit] - zref[hit]) / zref[hit]).max()) if hit.any() else 0.0


@gpu
@pytest.mark.parametrize("c", PANO_CASES, ids=_id)
def test_make_pano_and_scatter_min_word_for_word(ops, parity, c):
    k = pano_case(c)
    err = _check_pano(ops, parity, k["xyz"], k["rgb"], k["H"], k["W"], _id(c))
    parity("scatter_min_depth %s: zmin vs sqrt of the float64 norm (rel)" % _id(c), err, 2.5e-7)


@gpu
def test_make_pano_of_single_special_points(ops, parity):
    worst = 0.0
    for H, W, xyz, rgb in single_cases():
        worst = max(worst, _check_pano(ops, parity, xyz, rgb, H, W, (H, W, xyz.tolist())))
    parity("scatter_min_depth, one special point: zmin (rel)", worst, 2.5e-7)


def _c2i_points():
    """the 33 x 64 case's points, 2000 random directions at magnitudes 1e-6 .. 1e3, axis and seam points (last six rows)"""
    rng = np.random.default_rng(31)
    mag = np.concatenate([10.0 ** rng.uniform(-6, 3, 1990), [1e-6] * 5, [1e3] * 5])
    d = rng.normal(size=(2000, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * mag[:, None]).astype(F32)
    assert not ((pts[:, 1] == 0) & (pts[:, 0] == -F32(1e-6))).any()
    axis = np.array([[0, 0, 1], [0, 0, 1e-3], [0, 0, -1], [0, 0, -1e3], [-1, -0.0, 0], [-1, 0.0, 0]], F32)
    return np.concatenate([pano_case(PANO_CASES[-1])["xyz"], pts, axis])


@gpu
def test_cloud2idx_against_float64(ops, parity):
    xyz = _c2i_points()
    out = ops.cloud2idx(T(xyz)).cpu().numpy()
    parity("cloud2idx vs float64 (abs), magnitudes 1e-6 .. 1e3", np.abs(out - om.cloud2idx(xyz)).max(), 5e-7)
    up, down, seam_neg, seam_pos = out[-6:-4], out[-4:-2], out[-2], out[-1]
    assert (up[:, 0] == 0).all() and (up[:, 1] == -1).all()                 # +z axis
    assert (down[:, 1] == 1).all()                                          # -z axis
    assert seam_neg[0] == 1 and seam_pos[0] == -1


@gpu
def test_cloud2idx_backward_on_every_point(ops, parity):
    base = _c2i_points()
    axis = np.array([[0, 0, 1], [0, 0, 1e-3], [0, 0, -1], [0, 0, -1e3], [0, 0, 0]], F32)
    xyz = np.concatenate([base, axis, axis])
    rng = np.random.default_rng(32)
    G = rng.normal(size=(len(xyz), 2)).astype(F32)
    G[-len(axis):, 0] = 0                                                  # phi's branch off: what is left in x and y is the rho branch
    got = ops.cloud2idx_backward(T(xyz), T(G)).cpu().numpy()
    ref, m32 = om.cloud2idx_backward(xyz, G), om.cloud2idx_backward(xyz, G, F32)
    scale = np.maximum(np.abs(ref), 1.0)
    rho0 = (xyz[:, 0] == 0) & (xyz[:, 1] == 0)
    assert rho0.sum() == 3 + 4 + 2 * len(axis)                             # (the constructed cloud's two axis points and its origin)
    gap = (np.abs(m32 - ref) / scale)[~rho0].max()
    parity("cloud2idx backward vs float64, regular points", (np.abs(got - ref) / scale)[~rho0].max(), 2 * gap + 1e-6, gap)
    assert np.isfinite(got).all()
    parity("cloud2idx backward vs float64, axis points (rho = 0)", (np.abs(got - ref) / scale)[rho0].max(), 2 * gap + 1e-6, gap)
    assert (got[-len(axis):, :2] == 0).all() and (got[rho0, 2] == 0).all()
    assert (np.abs(got[-2 * len(axis):-len(axis), 1]) > 0).all()           # (phi's branch is alive on the axis)


@gpu
def test_transform_cloud_against_float64(ops, oracle, parity):
    rng = np.random.default_rng(33)
    worst = 0.0
    for n in (1, 255, 257, 4099):
        xyz = (rng.normal(size=(n, 3)) * 3).astype(F32)
        t, ypr = rng.normal(size=3).astype(F32), rng.uniform(-4, 7, 3).astype(F32)
        out = ops.transform_cloud(T(xyz), T(t), T(ypr)).cpu().numpy()
        q = xyz.astype(F64) - t.astype(F64)
        ref = q @ oracle.rot_from_ypr(ypr.astype(F64), F64).T
        worst = max(worst, float((np.abs(out - ref) / np.abs(q).sum(1, keepdims=True)).max()))
    parity("transform_cloud vs float64 R (x - t), per component / L1 norm of q", worst, 5e-7)
    # an image of the transformed cloud: a constructed cloud taken to the world by the inverse pose and back by the device
    H, W = 16, 32
    k = om.pano_case(H, W, 1200, seed=34, specials=False)
    t, ypr = rng.normal(size=3).astype(F32), rng.uniform(-4, 7, 3).astype(F32)
    R = oracle.rot_from_ypr(ypr.astype(F64), F64)
    world = (k["xyz"].astype(F64) @ R + t.astype(F64)).astype(F32)
    model = ((world.astype(F64) - t.astype(F64)) @ R.T).astype(F32)
    row, col, frow, fcol = om.pano_pixels(model, H, W)
    assert 0.2 <= min(frow.min(), fcol.min()) and max(frow.max(), fcol.max()) <= 0.8 and om.depth_separation(model) >= om.DEPTH_GAP
    cam = ops.transform_cloud(T(world), T(t), T(ypr))
    a = ops.make_pano(cam, T(k["rgb"]), (H, W)).cpu().numpy()
    b = ops.make_pano(T(model), T(k["rgb"]), (H, W)).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(b, om.pano_image(om.make_pano_winners(model, H, W, row, col)[0], k["rgb"], H, W))


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 257, 2048 * 256 + 257])
def test_quantile_box_exact(ops, oracle, n):
    rng = np.random.default_rng(35 + n)
    xyz = rng.normal(size=(n, 3)).astype(F32)
    if n == 2:
        xyz = np.array([[-0.0, np.inf, 1], [0.0, -np.inf, 1]], F32)
    if n >= 3:
        xyz[: n // 3, 0] = 0.25                                             # ties
        xyz[0, 1], xyz[n - 1, 1] = np.inf, -np.inf
        xyz[n // 2:, 2] = np.where(np.arange(n - n // 2) % 2 == 0, F32(-0.0), F32(0.0))       # -0.0 next to +0.0, up to the last row
    if n > 2048 * 256:
        xyz[2048 * 256:, 0] = -7.0             # the loop's second trip holds the smallest x: without it every rank of x moves by 257
    for q in (0.05, 0.25, 0.5):
        box = ops.quantile_box(T(xyz), q).cpu().numpy().reshape(3, 2)
        assert np.array_equal(box, oracle.quantile_box(xyz, q)), (n, q)      # (by value: -0.0 == +0.0)
    for q in (0.0, 1.0):
        with pytest.raises(ops._lib.PiccoloHipError):
            ops.quantile_box(T(xyz), q)


FMT_CODE = {"f32": 0, "u8": 1, "f16": 2}


def _ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 (nothing contributes) got must be exactly 0"""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    assert (got[bound == 0] == 0).all() and (ref[bound == 0] == 0).all()
    return float((np.abs(got - ref)[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@gpu
@pytest.mark.parametrize("H,W", SAMPLE_SHAPES)
def test_sample_from_img_forward(ops, parity, H, W):
    import torch
    k = sample_case(H, W)
    for n in (257, 255, 1):
        c = k["coord"][:n]
        dec = k["decidable"][:n]
        ref, m32 = om.sample_from_img(k["imgk"], c), om.sample_from_img(k["imgk"], c, F32)
        gap = np.abs(m32 - ref).max()
        outs = {}
        for fmt in ("f32", "u8", "f16"):
            pano = ops.Pano(T(k["imgk"]), fmt=fmt)
            assert pano.fmt == FMT_CODE[fmt]
            outs[fmt] = ops.sample_from_img(pano, T(c))
            o = outs[fmt].cpu().numpy()
            parity("sample_from_img[%s] %dx%d n=%d vs float64 (abs)" % (fmt, H, W, n), np.abs(o - ref).max(), 2 * gap + 1e-7, gap)
            assert np.array_equal((o == 0)[dec], (ref == 0)[dec])            # the exact-zero pattern drives the loss mask
        assert torch.equal(outs["u8"].view(torch.int32), outs["f16"].view(torch.int32))
        # an image that is not k/255: float texels
        pano = ops.Pano(T(k["imgs"]))
        assert pano.fmt == FMT_CODE["f32"]
        ref, m32 = om.sample_from_img(k["imgs"], c), om.sample_from_img(k["imgs"], c, F32)
        gap = np.abs(m32 - ref).max()
        o = ops.sample_from_img(pano, T(c)).cpu().numpy()
        parity("sample_from_img[f32, not k/255] %dx%d n=%d vs float64 (abs)" % (H, W, n), np.abs(o - ref).max(), 2 * gap + 1e-7, gap)
        assert np.array_equal((o == 0)[dec], (ref == 0)[dec])


@gpu
@pytest.mark.parametrize("H,W", SAMPLE_SHAPES)
def test_sample_from_img_backward(ops, parity, H, W):
    import torch
    k = sample_case(H, W)
    lim = om.LIM32
    for n in (257, 255, 1):
        c, g, dec = k["coord"][:n], k["gout"][:n], k["decidable"][:n]
        inr = om.sample_taps(c, H, W)["inr"]
        for img, fmts in ((k["imgk"], ("f32", "u8", "f16")), (k["imgs"], ("f32",))):
            m64, m32 = om.sample_from_img_backward(img, c, g), om.sample_from_img_backward(img, c, g, F32)
            gap_c = np.abs(m32["grad_coord"] - m64["grad_coord"])[dec].max() if dec.any() else 0.0
            gcs = {}
            for fmt in fmts:
                pano = ops.Pano(T(img), fmt=fmt)
                tag = "sample backward[%s%s] %dx%d n=%d: " % (fmt, "" if img is k["imgk"] else ", not k/255", H, W, n)
                gc_t, gi = ops.sample_from_img_backward(pano, T(c), T(g), want_coord=True, want_img=True)
                gcs[fmt] = gc_t
                gc, gi = gc_t.cpu().numpy(), gi.cpu().numpy()
                if dec.any():
                    parity(tag + "grad_coord vs float64 (abs)", np.abs(gc - m64["grad_coord"])[dec].max(), 2 * gap_c + 1e-5, gap_c)
                assert (gc[~inr] == 0).all() and np.isfinite(gc).all()       # exactly no gradient outside the clip, as fp32 compares it
                at_edge = (np.abs(c) == lim) & (np.abs(m64["grad_coord"]) > 1e-3) & dec[:, None]
                assert (gc[at_edge] != 0).all()                              # ... and the clip passes it AT +-0.99
                if n == 257:
                    assert at_edge.any()
                parity(tag + "grad_img vs float64 / atomic-sum bound, worst texel", _ratio(gi, m64["grad_img"], m64["bound"]), 1.0,
                       _ratio(m32["grad_img"], m64["grad_img"], m64["bound"]))
                # one output at a time
                only_c, none_i = ops.sample_from_img_backward(pano, T(c), T(g), want_coord=True, want_img=False)
                assert none_i is None and torch.equal(only_c.view(torch.int32), gc_t.view(torch.int32))
            if "u8" in gcs:
                assert torch.equal(gcs["u8"].view(torch.int32), gcs["f16"].view(torch.int32))
    # the weights alone (gradient 1 in the first channel): what every row and column of the image receives, and what the clipped points
    # alone still contribute — nothing from a tap in the zero border shows up anywhere
    c = k["coord"]
    ones = np.zeros((len(c), 3), F32)
    ones[:, 0] = 1
    pano = ops.Pano(T(k["imgs"]))
    for sel, what in ((np.ones(len(c), bool), "all points"), (~om.sample_taps(c, H, W)["inr"].all(1), "clipped points only")):
        m64, m32 = om.sample_from_img_backward(k["imgs"], c[sel], ones[sel]), om.sample_from_img_backward(k["imgs"], c[sel], ones[sel], F32)
        _, gi = ops.sample_from_img_backward(pano, T(c[sel]), T(ones[sel]), want_coord=False, want_img=True)
        gi = gi.cpu().numpy().astype(F64)
        assert m64["grad_img"][:, :, 0].sum() > 1.0 and (gi[:, :, 1:] == 0).all()
        for axis, name in ((1, "row"), (0, "column")):               # (the texels' bounds add up along a row or column)
            parity("sample backward %dx%d, %s: %s sums of the weights / summed atomic-sum bounds" % (H, W, what, name),
                   _ratio(gi[:, :, 0].sum(axis), m64["grad_img"][:, :, 0].sum(axis), m64["bound"][:, :, 0].sum(axis)), 1.0,
                   _ratio(m32["grad_img"][:, :, 0].astype(F64).sum(axis), m64["grad_img"][:, :, 0].sum(axis), m64["bound"][:, :, 0].sum(axis)))


@gpu
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (16, 32)])
def test_sample_backward_on_dyadic_inputs_is_exact(ops, H, W):
    """Power-of-two sizes, coordinates at quarter texels strictly inside the clip, gradients in eighths: every weight, contribution and
    partial sum is exact in fp32, so grad_img EQUALS the float64 model whatever the order of the atomics, and the run that asks for the
    image gradient alone equals the run that asks for both."""
    import torch
    rng = np.random.default_rng(36 + H + W)
    n = 257
    qx, qy = rng.integers(1, 4 * W - 1, n), rng.integers(1, 4 * H - 1, n)                     # quarter-texel positions, in (-0.99, 0.99)
    c = np.stack([qx / (2.0 * W) - 1.0, qy / (2.0 * H) - 1.0], 1).astype(F32)
    assert (np.abs(c) < om.LIM32).all()
    g = (rng.integers(-32, 33, (n, 3)) / 8.0).astype(F32)
    img = om.levels_image(rng.integers(0, 256, (H, W, 3)))
    m = om.sample_from_img_backward(img, c, g)
    pano = ops.Pano(T(img), fmt="f32")
    gc, gi = ops.sample_from_img_backward(pano, T(c), T(g), want_coord=True, want_img=True)
    assert np.array_equal(gi.cpu().numpy().astype(F64), m["grad_img"])
    none_c, only_i = ops.sample_from_img_backward(pano, T(c), T(g), want_coord=False, want_img=True)
    assert none_c is None and torch.equal(only_i, gi)


@gpu
def test_sample_backward_many_points_into_few_texels(ops, parity):
    """4096 points on a 2 x 3 image: float atomics into six texels, inside the fp32 summation bound per texel channel"""
    H, W, n = 2, 3, 4096
    rng = np.random.default_rng(37)
    c = rng.uniform(-1.2, 1.2, (n, 2)).astype(F32)
    g = rng.normal(size=(n, 3)).astype(F32)
    img = (rng.uniform(0, 1, (H, W, 3)) * 0.93).astype(F32)
    m = om.sample_from_img_backward(img, c, g)
    assert m["count"].min() >= 500
    _, gi = ops.sample_from_img_backward(ops.Pano(T(img)), T(c), T(g), want_coord=False, want_img=True)
    bound = (m["count"][:, :, None] + 3) * 2.0 ** -24 * m["asum"]
    parity("sample backward, 4096 points on 2x3: grad_img vs float64 / ((m + 3) 2^-24 sum of abs contributions), worst texel",
           (np.abs(gi.cpu().numpy() - m["grad_img"]) / bound).max(), 1.0)
