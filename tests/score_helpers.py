"""Reference semantics of the score maps (csrc/pcl_score.hip) for tests/test_score_maps.py — not a test module.  Plain numpy: the block
of a point comes from hist_helpers' projection (float64 unless asked otherwise), the sums run over the poses in ascending order in
float32, one float32 division at the end.  The rules (include/piccolo_hip.h, pcl_score_maps / pcl_score_weights):
    valid(k, j) = nproj[k][j] > 0 and nimg[j] > 0
    a point's pixel is the render's centre pixel (truncate, clamp, no wrap); h = row // bh, w = col // bw; it is in scored block
    (h - 1) nsw + w iff 1 <= h <= nsh - 2 and w < nsw, else in none
    score2d[j] = sum over the valid k of inter[k][j] / their number; score3d[p] = sum over the poses k where p is in a scored block j with
    valid(k, j) of inter[k][j] / their number; -1 where the number is 0; a pose that is not finite casts no vote
    weights: lo, hi over the points with count >= min_count; w = clamp(fma(1 - floor, (s - lo) / (hi - lo), floor), 0, 1); 1 for a point
    with fewer votes, for every point when none voted or hi == lo; padding 0"""
import types
from fractions import Fraction

import numpy as np

import hist_helpers as hh

F32 = np.float32
VARIANTS = ("all_k", "fold_rows", "fold_cols", "count_invalid")
CASE_NAMES = ("R1", "R2", "R5", "R6a", "empty")
UNDECIDED_CAP = 0.03

_SCENES = {}


def scene(name):
    """the case's decisive scene of hist_helpers, built once per session"""
    if name not in _SCENES:
        _SCENES[name] = hh.build_scene(**hh.CASES[name])
    return _SCENES[name]


def pixel_blocks(H, W, nsh, nsw, variant=None):
    """(H * W,) scored block of every pixel, -1 for none: hist_helpers.block_of, or a planted variant of it"""
    if variant not in ("fold_rows", "fold_cols"):
        return hh.block_of(H, W, nsh, nsw)
    bh, bw = H // nsh, W // nsw
    r, c = np.divmod(np.arange(H * W), W)
    h, w = r // bh, c // bw
    if variant == "fold_rows":
        h = np.clip(h, 1, nsh - 2)
    else:
        w = np.minimum(w, nsw - 1)
    ok = (h >= 1) & (h <= nsh - 2) & (w < nsw)
    return np.where(ok, (h - 1) * nsw + w, -1)


def coords(xyz, trans, rot, H, W, dtype=np.float64):
    """(rowf, colf), each (K, n): the fractional pixel coordinates of every point for every pose; NaN rows for a pose that is not finite"""
    K, n = len(trans), len(xyz)
    rowf, colf = np.full((K, n), np.nan, dtype), np.full((K, n), np.nan, dtype)
    for k in range(K):
        if np.isfinite(trans[k]).all() and np.isfinite(rot[k]).all():
            rowf[k], colf[k], _ = hh.project(hh.camera_points(xyz, trans[k], rot[k], dtype), H, W)
    return rowf, colf


def point_blocks(xyz, trans, rot, H, W, nsh, nsw, dtype=np.float64, variant=None):
    """(K, n) scored block of every point for every pose, -1 for none (and for every point of a pose that is not finite)"""
    of_pixel = pixel_blocks(H, W, nsh, nsw, variant)
    rowf, colf = coords(xyz, trans, rot, H, W, dtype)
    out = np.full(rowf.shape, -1, np.int64)
    for k in range(len(trans)):
        if not np.isnan(rowf[k]).any():
            row, col = hh.pixels(rowf[k], colf[k], H, W)
            out[k] = of_pixel[row * W + col]
    return out


def maps_model(blk, inter, nproj, nimg, variant=None):
    """blk (K, n) from point_blocks, inter / nproj (K, nblk), nimg (nblk,) -> namespace(score3d (n,) float32, count3d (n,) int32, score2d
    (nblk,), count2d (nblk,)); sequential float32 sums over the poses in ascending order"""
    assert variant is None or variant in VARIANTS
    inter = np.asarray(inter, F32)
    K, n = blk.shape
    nblk = inter.shape[1]
    valid = (np.asarray(nproj) > 0) & (np.asarray(nimg)[None, :] > 0)
    sum2, cnt2 = np.zeros(nblk, F32), np.zeros(nblk, np.int32)
    sum3, cnt3 = np.zeros(n, F32), np.zeros(n, np.int32)
    for k in range(K):
        m = valid[k]
        sum2[m] = sum2[m] + inter[k][m]
        cnt2[m] += 1
        j = blk[k]
        vote = j >= 0
        if variant != "count_invalid":
            vote = vote & valid[k][np.maximum(j, 0)]
        sum3[vote] = sum3[vote] + inter[k][j[vote]]
        cnt3[vote] += 1
    if variant == "all_k":
        cnt2, cnt3 = np.full(nblk, K, np.int32), np.full(n, K, np.int32)

    def mean(s, c):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = s / c.astype(F32)
        assert q.dtype == F32
        return np.where(c > 0, q, F32(-1))

    return types.SimpleNamespace(score3d=mean(sum3, cnt3), count3d=cnt3, score2d=mean(sum2, cnt2), count2d=cnt2)


def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding, elementwise over float32 b (a, c float32 scalars).  a b is exact in float64; the float64 sum is
    rounded once more on its way to float32, which matters only when it sits exactly half way between two float32 values: those
    elements are decided with exact fractions."""
    a, c = F32(a), F32(c)
    b = np.asarray(b, F32)
    s = np.float64(a) * b.astype(np.float64) + np.float64(c)
    out = s.astype(F32)
    half = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    for i in np.nonzero(half)[0]:
        exact = Fraction(float(a)) * Fraction(float(b[i])) + Fraction(float(c))
        lo, hi = np.nextafter(out[i], F32(-np.inf)), np.nextafter(out[i], F32(np.inf))
        out[i] = min((out[i], lo, hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(np.asarray(v, F32).view(np.uint32)) & 1))
    return out


def weights_model(score, count, floor, min_count, stride):
    """-> (plane (stride,) float32, (lo, hi, voted))"""
    score, count = np.asarray(score, F32), np.asarray(count)
    n = len(score)
    plane = np.zeros(stride, F32)
    plane[:n] = 1
    voted = count >= min_count
    if not voted.any():
        return plane, (F32(0), F32(0), 0)
    lo, hi = score[voted].min(), score[voted].max()
    if hi != lo:
        q = (score[voted] - lo) / (hi - lo)
        assert q.dtype == F32
        plane[:n][voted] = np.clip(fma32(F32(1) - F32(floor), q, F32(floor)), F32(0), F32(1))
    return plane, (lo, hi, int(voted.sum()))


def borders(H, W, nsh, nsw):
    """the pixel coordinates at which the block of a point changes: first rows of the block rows 1 .. nsh - 1 (the scored region's two edges
    among them), first columns of the block columns 1 .. nsw (the last one: the remainder's edge)"""
    bh, bw = H // nsh, W // nsw
    return bh * np.arange(1, nsh), bw * np.arange(1, nsw + 1)


def undecided_points(xyz, trans, rot, H, W, nsh, nsw):
    """-> (undecided (n,) bool, delta, flips): a point is undecided when, for some pose, a float64 pixel coordinate lies within delta of a
    block border; delta = 3 x the largest float32-vs-float64 difference of the coordinates over the (point, pose) pairs that can reach
    the scored rows (hist_helpers' convention; the row coordinate's own gap is asserted below 1e-3 everywhere, so the others are far
    from every scored row in either arithmetic).  flips: the decided points whose float32 block differs from the float64 one, for any pose."""
    r64, c64 = coords(xyz, trans, rot, H, W, np.float64)
    r32, c32 = coords(xyz, trans, rot, H, W, np.float32)
    rel = hh.relevant(r64, hh.scored_rows(H, nsh))
    assert float(np.abs(r32 - r64).max()) < 1e-3
    delta = 3.0 * max(float(np.abs(r32 - r64)[rel].max()), float(np.abs(c32 - c64)[rel].max()))
    rb, cb = borders(H, W, nsh, nsw)
    near = (np.abs(r64[:, :, None] - rb[None, None, :]).min(axis=2) < delta) | (np.abs(c64[:, :, None] - cb[None, None, :]).min(axis=2) < delta)
    und = (rel & near).any(axis=0)
    b64 = point_blocks(xyz, trans, rot, H, W, nsh, nsw, np.float64)
    b32 = point_blocks(xyz, trans, rot, H, W, nsh, nsw, np.float32)
    flips = int(((b64 != b32).any(axis=0) & ~und).sum())
    return und, delta, flips
