"""Case builders, numpy references and the guard of tests/test_color_exact.py (csrc/pcl_color.hip) — not a
test module.

color_match is compared with oracle/color.py within MATCH_TOL (the 1e-6 of tests/test_color.py).  The device's sinf and numpy's
float32 sin differ in the last place of a row weight, so a case is only compared when the MODEL is not itself more sensitive than that:
THE GUARD evaluates the oracle a second time with every row weight moved one float32 ulp (up on even rows, down on odd rows) and
asserts that the two oracle results differ by at most MATCH_TOL / 2.  A case that breaks the guard is replaced by another input; it
is neither skipped nor given a wider tolerance.
color_mod (byte arithmetic), the counts of histogram and the template sort are compared exactly."""
import zlib

import numpy as np

from oracle import color as ocolor
from test_color import MATCH_TOL

F = np.float32

SMALL_SHAPES = [(2, 2), (2, 3), (3, 5), (9, 1), (16, 16), (17, 15),          # below one block
                (31, 33), (32, 32), (25, 41)]                                 # 1023, 1024, 1025 pixels
# 262 397 pixels: above 256 x 1024, the histogram kernels loop; 525 825 pixels: above 2048 x 256, the apply kernels loop
LARGE_SHAPES = [(257, 1021), (513, 1025)]
LEVEL_SETS = {
    "all": np.arange(256),
    "gaps": np.arange(7, 250, 3),            # absent levels everywhere: table[rank[b]] is not table[b]
    "ends": np.array([1, 2, 254, 255]),      # a gap in the middle, the top level present
    "low": np.array([3, 4, 5]),              # everything above absent
}
TEMPLATES = ("even1", "even2", "even3", "even257", "even1025", "quant4099", "equal100", "zeros_ones", "cont1025")
LARGE_TEMPLATES = ("even1025", "quant4099")


def case_seed(*parts):
    """a seed that depends on the case alone (never on the order the tests run in)"""
    return zlib.crc32(repr(parts).encode())


def level_image(seed, H, W, levels, black=0.15):
    """uint8 levels / 255 with about 15 % black pixels; some non-black pixel lies below row 0 (whose weight is 0)"""
    rng = np.random.default_rng(seed)
    levels = np.asarray(levels)
    img8 = rng.choice(levels.astype(np.uint8), size=(H, W, 3))
    img8[rng.random((H, W)) < black] = 0
    if H > 1 and not img8[1:].any():
        img8[-1, -1] = levels[-1]
    return img8.astype(F) / F(255)


# Inputs that broke the guard and were replaced (match_reference says which figure; all five the order of the float32 sums):
#   'ends' at the two large shapes: four levels share 2e5 / 4e5 pixels, and the oracle moves by 0.95e-6 - 2.1e-6 under the order of its
#       sums -> 99 % black pixels (650 / 1300 pixels per level; the loops still walk every pixel);
#   'ends' at 25 x 41 with the continuous template (6.6e-7) -> another seed.
MATCH_BLACK = {((257, 1021), "ends"): 0.99, ((513, 1025), "ends"): 0.99}
MATCH_RESEED = {((25, 41), "ends"): 1}


def match_image(H, W, levels_name):
    """the image of a color_match case: one per shape and level set, shared by the templates"""
    key = ((H, W), levels_name)
    return level_image(case_seed(H, W, levels_name, MATCH_RESEED.get(key, 0)), H, W, LEVEL_SETS[levels_name], MATCH_BLACK.get(key, 0.15))


def template(name, seed=0):
    """(n, 3) float32 point colours"""
    rng = np.random.default_rng([seed, len(name)])
    if name.startswith("even"):                  # a shuffle of n evenly spaced values per channel
        n = int(name[4:])
        v = ((np.arange(n) + 1) / (n + 1)).astype(F)
        return np.stack([rng.permutation(v) for _ in range(3)], 1)
    if name.startswith("quant"):                 # random levels k / 255: runs of n / 256 equal values
        return rng.integers(0, 256, size=(int(name[5:]), 3)).astype(F) / F(255)
    if name.startswith("cont"):
        return rng.random((int(name[4:]), 3)).astype(F)
    if name == "equal100":                       # one run that touches both ends
        return np.tile(np.array([[0.25, 0.5, 0.8125]], F), (100, 1))
    if name == "zeros_ones":                     # two runs: one touches position 0, the other n - 1
        return np.repeat(np.array([0, 1], F), [333, 667])[:, None].repeat(3, 1).copy()
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------- color_match
def moved_row_weights(H, W):
    """the oracle's own row weights, each moved one float32 ulp: up on even rows, down on odd rows"""
    w = ocolor.pixel_weights(H, W).reshape(H, W)[:, 0].copy()
    up, down = np.nextafter(w, F(np.inf)), np.nextafter(w, F(-np.inf))
    w[0::2], w[1::2] = up[0::2], down[1::2]
    return w


def match_reference(img, rgb):
    """(oracle result, the larger of the guard's two figures): asserts the guard.
    Second figure, same bound: the oracle adds a level's weights in float32 in pixel order (torch.bincount on the CPU); the device
    adds them exactly, and the reference on a GPU adds them in no fixed order.  So the oracle is evaluated once more on the image
    turned by 180 degrees with the row weights reversed — the same weights in every level, added in the opposite order — and must
    not move by more than MATCH_TOL / 2 either.  (A level with 10^5 pixels breaks this: its float32 sum is then some 1e-6 off.)"""
    H, W, _ = img.shape
    ref = ocolor.color_match(img, rgb)
    moved = ocolor.color_match(img, rgb, moved_row_weights(H, W))
    w = ocolor.pixel_weights(H, W).reshape(H, W)[:, 0]
    turned = ocolor.color_match(img[::-1, ::-1], rgb, w[::-1])[::-1, ::-1]
    gap, order = float(np.abs(ref - moved).max()), float(np.abs(ref - turned).max())
    assert gap <= MATCH_TOL / 2, "guard: the oracle moves by %.3e under one ulp of its row weights: choose another input" % gap
    assert order <= MATCH_TOL / 2, "guard: the oracle moves by %.3e under the order of its float32 sums: choose another input" % order
    return ref, max(gap, order)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


MONO_ULPS = 12


def check_match_invariants(img, out, rgb):
    """What holds whatever MATCH_TOL is: black pixels come back bit for bit; two pixels of one level in a channel get the same bits
    (hence no more distinct outputs than levels); per channel the map level -> output falls to its minimum and rises from there.
    (The reference's interpolation wraps: below the template's first quantile it interpolates from the template's LAST value, 360
    to the left, down to its first, so the map is non-increasing on those levels and non-decreasing on all others.  With a template
    of many distinct values the first quantile is 1 / n and the map is non-decreasing throughout.)
    The interpolant ((x - xs) fb + (xb - x) fs) / (xb - xs) is six float32 roundings (two differences, two products, a sum, a
    quotient; the denominator's is a seventh that both weights share), each at most 2^-24 of max |template|: two neighbouring levels
    whose exact values agree (a template of equal values, quantiles one ulp apart) may come out 12 x 2^-24 max |template| in the
    wrong order, in the oracle as on the device.  That is the slack of the monotonicity; nothing else has any."""
    slack = F(MONO_ULPS * 2.0 ** -24) * np.abs(np.asarray(rgb, F)).max()
    black = ~ocolor.nonblack_mask(img)
    assert np.array_equal(bits(out[black]), bits(img[black]))
    nb = ~black
    for c in range(3):
        lev = np.rint(img[..., c][nb] * F(255)).astype(np.int64)
        val = bits(out[..., c][nb])
        order = np.argsort(lev, kind="stable")
        lev, val = lev[order], val[order]
        same = lev[1:] == lev[:-1]
        assert (val[1:][same] == val[:-1][same]).all(), "channel %d: one level, two outputs" % c
        first = np.concatenate([[True], ~same]) if lev.size else np.zeros(0, bool)
        per_level = val[first].view(F)
        assert np.unique(val).size <= first.sum()
        if per_level.size:
            k = int(np.flatnonzero(per_level == per_level.min())[-1])
            assert (np.diff(per_level[:k + 1]) <= slack).all() and (np.diff(per_level[k:]) >= -slack).all(), "channel %d: not monotone" % c


# --------------------------------------------------------------------------------------------------- color_mod
def mod_image(kind, seed, H, W):
    rng = np.random.default_rng(seed)
    if kind == "levels":
        return level_image(seed, H, W, LEVEL_SETS["all"])
    if kind == "cont":                           # not k / 255: the truncations (int)(v * 255.f) decide
        img = rng.random((H, W, 3)).astype(F)
        img[rng.random((H, W)) < 0.15] = 0
        return img
    if kind == "edges":                          # exactly 0, 1, 1/255 and values just under 1/255 (black by the mask rule when in all three)
        under = np.nextafter(F(1) / F(255), F(0))
        vals = np.array([0, 1, F(1) / F(255), under, under * F(0.5), 0.5, np.nextafter(F(1), F(0))], F)
        img = rng.choice(vals, size=(H, W, 3))
        img[rng.random((H, W)) < 0.2] = under    # all three channels just under 1/255: black
        return img
    raise KeyError(kind)


def mod_colours(kind, seed, n):
    rng = np.random.default_rng(seed)
    if kind == "cont":
        return rng.random((n, 3)).astype(F)
    return rng.integers(0, 256, size=(n, 3)).astype(F) / F(255)


# --------------------------------------------------------------------------------------------------- histogram
def bin_sizes(channels):
    """ceil(255 / channels) in float32 (color_utils.py:86)"""
    return np.ceil(F(255) / np.asarray(channels, F)).astype(np.int64)


def ref_counts(img, mask, channels, unit):
    """raw counts of one image (color_utils.py:88-97), flat index r + c0 g + c0 c1 b; `unit`: the decision of `max <= 1`"""
    img = np.asarray(img, F)
    v = (img * F(255)).astype(np.int64) if unit else img.astype(np.int64)
    q = v[np.asarray(mask) != 0] // bin_sizes(channels)
    code = q[:, 0] + channels[0] * q[:, 1] + channels[0] * channels[1] * q[:, 2]
    nbins = int(np.prod(channels))
    assert code.size == 0 or (code.min() >= 0 and code.max() < nbins), "the case leaves the bins: the reference's reshape would raise"
    return np.bincount(code, minlength=nbins).astype(np.int64)


def ref_hist(img, mask, channels, normalize=True):
    """the unbatched form (color_utils.py:83-102): the image's own maximum decides the scale; hist / hist.sum(), one float32
    division per bin (NaN throughout for an empty mask: 0 / 0)"""
    h = ref_counts(img, mask, channels, np.asarray(img).max() <= 1).astype(F)
    if normalize:
        with np.errstate(invalid="ignore"):
            h = h / h.sum(dtype=F)
    return h


def ref_hist_batched(imgs, masks, channels, normalize=True):
    """the batched form (color_utils.py:83-89, 103-117): ONE maximum over the whole batch decides the scale; masked-out pixels are
    sent to bin 0 and taken off it again, i.e. not counted; hist / (hist.sum() + 1e-6)"""
    imgs = np.asarray(imgs, F)
    unit = imgs.max() <= 1
    out = []
    for im, m in zip(imgs, masks):
        h = ref_counts(im, m, channels, unit).astype(F)
        if normalize:
            h = h / (h.sum(dtype=F) + F(1e-6))
        out.append(h)
    return np.stack(out)


def hist_image(seed, H, W, unit, top=(255, 255, 255)):
    """integer colours 0..top per channel, as floats (unit: divided by 255), and a mask of about 60 %"""
    rng = np.random.default_rng(seed)
    img = np.stack([rng.integers(0, t + 1, size=(H, W)) for t in top], -1).astype(F)
    img[0, 0] = top                              # the maximum is attained
    mask = rng.random((H, W)) < 0.6
    mask[0, 0] = True
    return (img / F(255) if unit else img), mask


def ref_intersection(a, b):
    """float64 sum of the float32 minima, rounded once to float32, per row"""
    return np.minimum(np.asarray(a, F), np.asarray(b, F)).astype(np.float64).sum(-1).astype(F)
