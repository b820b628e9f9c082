"""The colour stage (csrc/pcl_color.hip) on ragged, tiny and degenerate inputs: ColorTemplate against a sort, color_match against
oracle/color.py within MATCH_TOL under the guard of tests/color_helpers.py, color_mod against the oracle exactly, histogram against a
numpy restatement of color_utils.py:68-144 exactly.

Shapes: below one block, 1023 / 1024 / 1025 pixels, 262 397 pixels (the 256 x 1024 histogram grid loops) and 525 825 pixels (the
2048 x 256 apply grid loops).  Two defects were found by these tests and fixed with them:
  * every non-black pixel in row 0 (weight sin(0) = 0; any image of one row): the quantiles were 0 / 0 and color_match wrote NaN into
    every non-black pixel (test_color_match_zero_total_weight: 3 of 3 cases failed on the parent, all of them with NaN);
  * the batched histogram took the scale (x 255 when max <= 1) from each image's own maximum; the reference asks the whole batch once
    (test_histogram_batched_scale_is_decided_by_the_batch[levels_0_1] failed on the parent; the [black] case cannot tell the two
    rules apart, 0 x 255 = 0, and is kept as the plain statement of the rule).
The largest |device - oracle| of color_match over the 340 compared images was 4.5e-7 (25 x 41, levels {1, 2, 254, 255}, the template
of 333 zeros and 667 ones) against MATCH_TOL = 1e-6; the guard's largest figure on them is 3.3e-7 (31 x 33, continuous template).

PLANTED MISTAKES.  Each was built once into a scratch copy of the library, and the 217 GPU tests of this file run against it:
  (a) table[rank[b]] -> table[b]: 71 failed — test_color_match_oracle (67 of 85), test_color_match_hand_made (3 of 3),
      test_template_cache_follows_the_tensor;
  (b) pcl_lower_bound_at returning hi - 1 when hi > 0: 55 failed — test_color_match_oracle (53), test_color_match_hand_made (1),
      test_template_cache_follows_the_tensor;
  (c) the row weight taken from h + 1: 72 failed — test_color_match_oracle (67), test_color_match_zero_total_weight (3 of 3),
      test_color_match_hand_made (1), test_template_cache_follows_the_tensor;
  (d) pcl_mod_hist_kernel ignoring `masked`: 32 failed — test_color_mod_oracle (26 of 27), test_color_mod_oracle_histogram_loop (3 of 3),
      test_color_mod_oracle_both_loops (2 of 2), test_color_mod_all_black;
  (e) the 4096-bin switch of pcl_histogram moved to `<`: NOT caught, and no comparison of results can catch it: at exactly 4096 bins
      the LDS kernel and the global-counter kernel are both in range and count the same pixels, so the change moves time, not
      values.  What the results do pin is each side of the switch: 16 x 16 x 16 (4096 bins) and 16 x 16 x 17 (4352) at every shape.
"""
import functools

import numpy as np
import pytest
import torch

import color_helpers as ch
from color_helpers import F, MATCH_TOL
from oracle import color as ocolor

gpu = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def cu():
    from piccolo_amd import color_utils as c
    from piccolo_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return c


@functools.lru_cache(maxsize=None)
def colours(name):
    """(numpy colours, the same on the device): one tensor per template for the whole module, so color_utils' cache sees one object"""
    rgb = ch.template(name)
    return rgb, T(rgb)


def compare_match(cu, img, rgb, rgb_t, ref):
    out = N(cu.color_match(T(img), rgb_t))
    err = float(np.abs(out - ref).max()) if out.size else 0.0
    assert not np.isnan(out).any()
    assert err <= MATCH_TOL, "color_match: %.3e from the oracle" % err
    ch.check_match_invariants(img, out, rgb)
    return err


# ------------------------------------------------------------------------------------------------------- CPU
def test_oracle_row_weights_default_is_unchanged():
    """the oracle with its own row weights passed in explicitly is the oracle, bit for bit; the moved weights differ in every row"""
    for (H, W) in ((3, 5), (25, 41)):
        img, rgb = ch.match_image(H, W, "all"), ch.template("cont1025")
        w = ocolor.pixel_weights(H, W).reshape(H, W)
        assert (w == w[:, :1]).all()
        assert np.array_equal(ch.bits(ocolor.color_match(img, rgb)), ch.bits(ocolor.color_match(img, rgb, w[:, 0])))
        assert (ch.moved_row_weights(H, W) != w[:, 0]).all()


def test_oracle_returns_a_weightless_image_unchanged():
    rgb = ch.template("even257")
    black = np.zeros((4, 4, 3), F)
    assert np.array_equal(ocolor.color_match(black, rgb), black)
    for img in zero_weight_images().values():
        assert np.array_equal(ch.bits(ocolor.color_match(img, rgb)), ch.bits(img))


@pytest.mark.parametrize("shape", ch.SMALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_oracle_passes_the_guard_and_the_invariants(shape):
    """every small case on the CPU: the guard holds and the oracle itself has the properties asserted of the device"""
    for t in ch.TEMPLATES:
        rgb = ch.template(t)
        for ln in ch.LEVEL_SETS:
            img = ch.match_image(*shape, ln)
            ref, _ = ch.match_reference(img, rgb)
            ch.check_match_invariants(img, ref, rgb)


def test_histogram_restatement_known_answers():
    """the numpy restatement itself: bin sizes, the flat index, the two scale rules"""
    assert ch.bin_sizes([32, 32, 32]).tolist() == [8, 8, 8] and ch.bin_sizes([2, 3, 5]).tolist() == [128, 85, 51]
    assert ch.bin_sizes([16, 16, 17]).tolist() == [16, 16, 15] and ch.bin_sizes([1, 1, 1]).tolist() == [255, 255, 255]
    img = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 203], [1, 1, 1]]], F)
    m = np.ones((2, 2), bool)
    h = ch.ref_counts(img, m, [5, 5, 5], unit=False)
    assert h[5] == 1 and h[25] == 1 and h[75] == 1 and h[0] == 1 and h.sum() == 4          # red 255 -> q 5: the flat index decides
    low = np.array([[[1, 0, 0], [0, 1, 1]], [[0, 0, 0], [1, 1, 1]]], F)                    # levels 0 and 1: alone, unit range
    alone = ch.ref_hist(low, m, [256, 2, 2], normalize=False)
    assert alone[255] == 1 and alone[768] == 1 and alone[0] == 1 and alone[1023] == 1
    both = ch.ref_hist_batched(np.stack([low, img]), np.stack([m, m]), [256, 2, 2], normalize=False)
    assert both[0][0] == 2 and both[0][1] == 2 and both[0].sum() == 4                       # in a 0..255 batch: not scaled
    assert both[1][255] == 1 and both[1][256] == 1 and both[1][512] == 1 and both[1][1] == 1


# ------------------------------------------------------------------------------------------- ColorTemplate
TEMPLATE_SIZES = (1, 2, 3, 255, 256, 257, 1025, 100_003)


def sort_input(content, n):
    rng = np.random.default_rng(ch.case_seed("sort", content, n))
    if content == "cont":
        return rng.random((n, 3)).astype(F)
    if content == "runs":                        # levels k / 255 with long runs
        return (rng.integers(0, 8, size=(n, 3)) * 36).astype(F) / F(255)
    if content == "equal":
        return np.full((n, 3), 0.3, F)
    special = np.array([0.0, -0.0, 1.0, -0.5, 1.5, -3.0, 2.0, np.nextafter(F(0), F(1)), -np.nextafter(F(0), F(1))], F)
    return np.stack([np.resize(rng.permutation(special), n) for _ in range(3)], 1)


@gpu
@pytest.mark.parametrize("content", ("cont", "runs", "equal", "special"))
@pytest.mark.parametrize("n", TEMPLATE_SIZES)
def test_template_is_the_sorted_colours(cu, n, content):
    from piccolo_amd import ops
    rgb = sort_input(content, n)
    t = ops.ColorTemplate(T(rgb))
    data = N(t.data)
    assert t.n == n and data.shape == (3, n)
    for c in range(3):
        assert np.array_equal(data[c], np.sort(rgb[:, c]))          # values: 0.0 == -0.0


@gpu
def test_template_cache_follows_the_tensor(cu):
    """the same tensor: the same template object; changed in place: a new template, and color_match follows the new colours"""
    img = ch.match_image(17, 15, "all")
    rgb = ch.template("cont1025").copy()
    rgb_t = T(rgb)
    t1 = cu._template(rgb_t)
    assert cu._template(rgb_t) is t1
    compare_match(cu, img, rgb, rgb_t, ch.match_reference(img, rgb)[0])
    assert cu._template(rgb_t) is t1
    rgb_t.mul_(0.5).add_(0.25)
    rgb2 = N(rgb_t)
    t2 = cu._template(rgb_t)
    assert t2 is not t1 and cu._template(rgb_t) is t2
    assert np.array_equal(N(t2.data), np.sort(rgb2, 0).T)
    ref2 = ch.match_reference(img, rgb2)[0]
    assert np.abs(ref2 - ch.match_reference(img, rgb)[0]).max() > 0.1          # the two answers are far apart
    compare_match(cu, img, rgb2, rgb_t, ref2)


# --------------------------------------------------------------------------------------------- color_match
MATCH_PAIRS = [(s, t) for s in ch.SMALL_SHAPES for t in ch.TEMPLATES] + [(s, t) for s in ch.LARGE_SHAPES for t in ch.LARGE_TEMPLATES]


@gpu
@pytest.mark.parametrize("shape,tname", MATCH_PAIRS, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_color_match_oracle(cu, shape, tname):
    rgb, rgb_t = colours(tname)
    for ln in ch.LEVEL_SETS:
        img = ch.match_image(*shape, ln)
        ref, _ = ch.match_reference(img, rgb)
        err = compare_match(cu, img, rgb, rgb_t, ref)
        print("color_match %dx%d %s %s: %.3e" % (*shape, tname, ln, err))


def hand_made_images():
    one = np.zeros((4, 4, 3), F)
    one[2, 1] = [F(3) / F(255), 0, 1]                            # one non-black pixel; a channel of it at level 0
    faint = np.zeros((6, 4, 3), F)
    faint[3, 2] = [0, F(1) / F(255), 0]                          # non-black by one channel at 1 / 255
    faint[1, 1] = [F(7) / F(255), F(9) / F(255), 0]
    flat = np.zeros((6, 4, 3), F)
    flat[1:5, :3] = F(77) / F(255)                               # every non-black pixel at one level
    return {"one_pixel": one, "faint_pixel": faint, "one_level": flat}


@gpu
@pytest.mark.parametrize("name", sorted(hand_made_images()))
def test_color_match_hand_made(cu, name):
    img = hand_made_images()[name]
    for tname in ch.TEMPLATES:
        rgb, rgb_t = colours(tname)
        compare_match(cu, img, rgb, rgb_t, ch.match_reference(img, rgb)[0])


@gpu
def test_color_match_all_black(cu):
    """no non-black pixel: the image comes back bit for bit and nothing is flagged (values under 1 / 255 are black by the mask rule)"""
    rgb_t = colours("cont1025")[1]
    under = np.nextafter(F(1) / F(255), F(0))
    for img in (np.zeros((4, 4, 3), F), np.zeros((25, 41, 3), F), np.full((3, 5, 3), under, F), np.full((32, 33, 3), -0.0, F)):
        out = N(cu.color_match(T(img), rgb_t))
        assert np.array_equal(ch.bits(out), ch.bits(img))


def zero_weight_images():
    row = ch.level_image(3, 1, 7, ch.LEVEL_SETS["all"])          # H = 1: the only row has weight sin(0)
    top = np.zeros((5, 7, 3), F)
    top[0] = ch.level_image(4, 1, 7, ch.LEVEL_SETS["gaps"])[0]
    col = np.zeros((8, 1, 3), F)
    col[0, 0] = [F(200) / F(255), 0, F(13) / F(255)]
    return {"one_row": row, "row0_of_5x7": top, "row0_of_8x1": col}


@gpu
@pytest.mark.parametrize("name", sorted(zero_weight_images()))
def test_color_match_zero_total_weight(cu, name):
    """every non-black pixel in row 0: total weight 0.  The reference raises (0 / 0 quantiles); the device returns the image."""
    img = zero_weight_images()[name]
    assert ocolor.nonblack_mask(img).any()
    for tname in ("even1", "quant4099", "cont1025"):
        out = N(cu.color_match(T(img), colours(tname)[1]))
        assert not np.isnan(out).any()
        assert np.array_equal(ch.bits(out), ch.bits(img))


@gpu
@pytest.mark.parametrize("where", ("first", "middle", "last"))
@pytest.mark.parametrize("what", ("between", "above_one", "negative", "nan"))
def test_color_match_flags_a_value_that_is_no_level(cu, what, where):
    """one bad channel in one pixel of a 25 x 41 image, wherever it lies, reaches the flag"""
    img = ch.match_image(25, 41, "all").copy()
    r, c = {"first": (0, 0), "middle": (12, 20), "last": (24, 40)}[where]
    bad = {"between": 0.5003, "above_one": np.nextafter(F(1), F(2)), "negative": -0.2, "nan": np.nan}[what]
    img[r, c] = [F(127) / F(255), bad, F(127) / F(255)]
    with pytest.raises(ValueError):
        cu.color_match(T(img), colours("cont1025")[1])


# ----------------------------------------------------------------------------------------------- color_mod
MOD_BINS = (2, 3, 255, 256, 257, 4095, 4096)
MOD_COLOURS = [(k, n) for n in (1, 2, 255, 1025) for k in ("cont", "levels")]


def compare_mod(cu, img, rgb, bins):
    ti, tr = T(img), T(rgb)
    oi, orgb = cu.color_mod(ti, tr, bins)
    ri, rrgb = ocolor.color_mod(img, rgb, bins)
    assert np.array_equal(N(oi), ri), "image, %d bins" % bins                   # byte arithmetic: exact
    assert np.array_equal(N(orgb), rrgb), "colours, %d bins" % bins
    assert np.array_equal(ch.bits(N(ti)), ch.bits(img)) and np.array_equal(ch.bits(N(tr)), ch.bits(rgb))          # inputs unchanged
    black = ~ocolor.nonblack_mask(img)
    assert np.array_equal(ch.bits(N(oi)[black]), ch.bits(img[black]))
    return N(oi)


@gpu
@pytest.mark.parametrize("kind", ("levels", "cont", "edges"))
@pytest.mark.parametrize("shape", ch.SMALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_color_mod_oracle(cu, shape, kind):
    """every num_bins at every small shape and image kind; the colour sets take turns (each meets every num_bins over the shapes)"""
    img = ch.mod_image(kind, ch.case_seed("mod", shape, kind), *shape)
    turn = ch.SMALL_SHAPES.index(shape) + ("levels", "cont", "edges").index(kind)
    for i, bins in enumerate(MOD_BINS):
        ckind, n = MOD_COLOURS[(turn + i) % len(MOD_COLOURS)]
        compare_mod(cu, img, ch.mod_colours(ckind, ch.case_seed("modc", ckind, n), n), bins)


@gpu
@pytest.mark.parametrize("kind", ("levels", "cont", "edges"))
def test_color_mod_oracle_histogram_loop(cu, kind):
    """262 397 pixels: the masked histogram kernel walks its grid-stride loop"""
    img = ch.mod_image(kind, ch.case_seed("mod", kind), 257, 1021)
    for bins, (ckind, n) in ((2, ("cont", 1025)), (256, ("levels", 255)), (4096, ("cont", 2))):
        compare_mod(cu, img, ch.mod_colours(ckind, 5, n), bins)


@gpu
@pytest.mark.parametrize("kind,ckind,bins", [("cont", "levels", 256), ("levels", "cont", 4096)])
def test_color_mod_oracle_both_loops(cu, kind, ckind, bins):
    """525 825 pixels and 524 288 + 257 colours: the histogram and the apply kernels loop over the image and over the colours"""
    img = ch.mod_image(kind, ch.case_seed("mod", kind), 513, 1025)
    compare_mod(cu, img, ch.mod_colours(ckind, 6, 524_288 + 257), bins)


@gpu
def test_color_mod_all_black(cu):
    """no non-black pixel: the table comes from the colours alone (the oracle's, exactly), the image comes back bit for bit"""
    under = np.nextafter(F(1) / F(255), F(0))
    for img in (np.zeros((4, 4, 3), F), np.full((25, 41, 3), under, F)):
        for bins in (2, 256, 4096):
            out = compare_mod(cu, img, ch.mod_colours("cont", 7, 1025), bins)
            assert np.array_equal(ch.bits(out), ch.bits(img))


@gpu
@pytest.mark.parametrize("bins", (0, 1, 4097))
def test_color_mod_refuses_bin_counts_outside_2_to_4096(cu, bins):
    from piccolo_amd import _lib
    img = ch.mod_image("levels", 1, 3, 5)
    with pytest.raises(_lib.PiccoloHipError):
        cu.color_mod(T(img), T(ch.mod_colours("cont", 7, 2)), bins)


# ----------------------------------------------------------------------------------------------- histogram
HIST_SHAPES = [(2, 2), (3, 5), (31, 33), (32, 32), (25, 41), (257, 1021)]
# channels -> the largest colour per channel.  The reference's flat index r + c0 g + c0 c1 b is only a bin while it stays below
# c0 c1 c2 (torch's reshape raises otherwise), so colours stop where 255 // ceil(255 / c) would reach c — except in the [5, 5, 5] case,
# where red and green DO reach 255 (q = 5 = c: the flat index carries into the next channel's bin) and blue stops at 203 (q <= 3), which
# keeps 5 + 25 + 75 below 125.
HIST_CHANNELS = {
    "1x1x1": ([1, 1, 1], (254, 254, 254)),
    "2x3x5": ([2, 3, 5], (255, 254, 254)),
    "16x16x16": ([16, 16, 16], (255, 255, 255)),          # 4096 bins: the last size counted in LDS
    "16x16x17": ([16, 16, 17], (255, 255, 254)),          # 4352 bins: the first size counted in global memory
    "5x5x5_carry": ([5, 5, 5], (255, 255, 203)),
}


@gpu
@pytest.mark.parametrize("cname", sorted(HIST_CHANNELS))
@pytest.mark.parametrize("shape", HIST_SHAPES, ids=lambda s: "%dx%d" % s)
def test_histogram_counts(cu, shape, cname):
    channels, top = HIST_CHANNELS[cname]
    for unit in (True, False):
        img, mask = ch.hist_image(ch.case_seed("hist", shape, cname, unit), *shape, unit, top)
        raw = N(cu.histogram(T(img), T(mask), channels, normalize=False))
        assert raw.shape == tuple(channels)
        want = ch.ref_counts(img, mask, channels, unit)
        assert np.array_equal(raw.reshape(-1), want.astype(F)) and raw.sum(dtype=np.float64) == mask.sum()
        h = N(cu.histogram(T(img), T(mask), channels))
        assert np.array_equal(h.reshape(-1), ch.ref_hist(img, mask, channels))              # one float32 division per bin
    # batched: the same images as a batch of two (both of one range)
    a, ma = ch.hist_image(ch.case_seed("hb", shape, cname, 0), *shape, False, top)
    b, mb = ch.hist_image(ch.case_seed("hb", shape, cname, 1), *shape, False, top)
    imgs, masks = np.stack([a, b]), np.stack([ma, mb])
    hb = N(cu.histogram(T(imgs), T(masks), channels))
    assert hb.shape == (2, *channels)
    assert np.array_equal(hb.reshape(2, -1), ch.ref_hist_batched(imgs, masks, channels))
    rawb = N(cu.histogram(T(imgs), T(masks), channels, normalize=False))
    assert np.array_equal(rawb.reshape(2, -1), ch.ref_hist_batched(imgs, masks, channels, normalize=False))


@gpu
@pytest.mark.parametrize("shape", [(3, 5), (25, 41)], ids=lambda s: "%dx%d" % s)
def test_histogram_scale_rule(cu, shape):
    """max == 1.0: unit range (x 255); max == nextafter(1, 2): a 0..255 image whose values truncate to 0 or 1; all zeros: unit range"""
    channels = [256, 2, 2]                                      # red in bins of one level: 0, 1 and 255 are told apart
    rng = np.random.default_rng(ch.case_seed("scale", shape))
    base = rng.random((*shape, 3)).astype(F)                    # continuous, below 1
    mask = np.ones(shape, bool)
    one, over, zero = base.copy(), base.copy(), np.zeros((*shape, 3), F)
    one[0, 0, 0] = 1.0
    over[0, 0, 0] = np.nextafter(F(1), F(2))
    for img in (one, over, zero):
        raw = N(cu.histogram(T(img), T(mask), channels, normalize=False)).reshape(-1)
        assert np.array_equal(raw, ch.ref_counts(img, mask, channels, img.max() <= 1).astype(F))
        assert np.array_equal(N(cu.histogram(T(img), T(mask), channels)).reshape(-1), ch.ref_hist(img, mask, channels))
    # what the rule means: `over` is a 0..255 image whose values truncate to 0 (all but one) and 1
    want = ch.ref_counts(over, mask, channels, False)
    assert want[0] == mask.sum() - 1 and want[1] == 1
    assert ch.ref_counts(one, mask, channels, True)[255::256].sum() == 1 and ch.ref_counts(zero, mask, channels, True)[0] == mask.sum()


@gpu
@pytest.mark.parametrize("cname", ("16x16x16", "16x16x17"))
def test_histogram_empty_mask(cu, cname):
    channels, top = HIST_CHANNELS[cname]
    img, _ = ch.hist_image(1, 25, 41, False, top)
    mask = np.zeros((25, 41), bool)
    assert not N(cu.histogram(T(img), T(mask), channels, normalize=False)).any()
    assert np.isnan(N(cu.histogram(T(img), T(mask), channels))).all()                      # the reference's 0 / 0
    imgs, masks = np.stack([img, img]), np.stack([mask, mask])
    hb = N(cu.histogram(T(imgs), T(masks), channels))
    assert hb.shape == (2, *channels) and not hb.any()                                      # 0 / (0 + eps)
    half = np.stack([mask, ~mask])
    assert np.array_equal(N(cu.histogram(T(imgs), T(half), channels)).reshape(2, -1), ch.ref_hist_batched(imgs, half, channels))


@gpu
@pytest.mark.parametrize("first", ("levels_0_1", "black"))
def test_histogram_batched_scale_is_decided_by_the_batch(cu, first):
    """color_utils.py:88 asks `tgt_img.max() <= 1` of the whole batch: in a 0..255 batch an image that holds only levels 0 and 1 (or is
    black) is NOT scaled by 255, although alone it would be."""
    channels = [8, 8, 8]
    rng = np.random.default_rng(11)
    shape = (25, 41)
    low = rng.integers(0, 2, size=(*shape, 3)).astype(F) if first == "levels_0_1" else np.zeros((*shape, 3), F)
    full, m1 = ch.hist_image(12, *shape, False)
    m0 = rng.random(shape) < 0.6
    imgs, masks = np.stack([low, full]), np.stack([m0, m1])
    want = ch.ref_hist_batched(imgs, masks, channels)
    assert want[0].reshape(-1)[0] > 0.99                                                   # unscaled: every pixel of `low` in bin 0
    got = N(cu.histogram(T(imgs), T(masks), channels)).reshape(2, -1)
    assert np.array_equal(got, want)
    assert np.array_equal(N(cu.histogram(T(imgs), T(masks), channels, normalize=False)).reshape(2, -1),
                          ch.ref_hist_batched(imgs, masks, channels, normalize=False))
    # alone, the same image is a unit-range image: scaled (levels 0 and 255)
    alone = N(cu.histogram(T(low), T(m0), channels, normalize=False)).reshape(-1)
    assert np.array_equal(alone, ch.ref_counts(low, m0, channels, True).astype(F))
    # a unit-range batch is scaled as a whole
    unit = imgs / F(255)
    assert np.array_equal(N(cu.histogram(T(unit), T(masks), channels)).reshape(2, -1), ch.ref_hist_batched(unit, masks, channels))


@gpu
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("nbins", (1, 27, 257, 4352))
def test_histogram_intersection(cu, nbins, batch):
    """the float64 sum of the float32 minima rounded once; the kernel adds the same doubles in another order: one float32 ulp"""
    shape = {1: (1, 1, 1), 27: (3, 3, 3), 257: (257, 1, 1), 4352: (16, 16, 17)}[nbins]
    rng = np.random.default_rng(ch.case_seed("inter", nbins, batch))
    a = rng.random((batch, *shape)).astype(F)
    b = rng.random((batch, *shape)).astype(F)
    a, b = a / a.sum(), b / b.sum()
    want = ch.ref_intersection(a.reshape(batch, -1), b.reshape(batch, -1))
    got = N(cu.histogram_intersection(T(a), T(b)))
    assert got.shape == (batch,) and (np.abs(got - want) <= np.spacing(want)).all()
    one = N(cu.histogram_intersection(T(a[0]), T(b[0])))
    assert one.shape == () and abs(one - want[0]) <= np.spacing(want[0])
