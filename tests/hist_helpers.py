"""Reference semantics of the render + histogram stage (csrc/pcl_hist.hip; make_pano / scatter-min of csrc/pcl_ops.hip) for
tests/test_hist_exact.py — not a test module.  Plain numpy, float64: a restatement of utils.py:134-205, 510-588 and
color_utils.py:68-144.

Everything in the stage is an integer until the last division: with a decided winner per pixel the block histograms are exact counts.
The model, per candidate pose and point (the points in PACKED order, so that a point's index is its packed slot):
    p = R (x - t)            pixel = clamp(trunc(make_pano's fractional coordinates))  (no wrap at the seam)       depth = |p|
    nine passes in oracle.PANO_PASSES order, each clamped to the image; a pixel's winner: latest pass, then nearest, then largest slot
    colour code = trunc(fp32(rgb) * fp32(255)) // 32 per channel; a winner that is exactly black leaves the pixel unrendered (and
    still hides what is behind it)
    blocks bh = H // nsh, bw = W // nsw; only block rows 1 .. nsh - 2 are scored, pixels at and beyond nsh * bh / nsw * bw are in no block
    candidate histograms: pixels where render and query are both non-black; query histograms: the query's own non-black pixels
    inter = sum min(h / sum h, q / sum q); the slot rule with its carry-over; NaN clean-up; score = sum slots / (nsh * nsw)
DECISIVE SCENES.  A kernel that works in fp32 may put a point within a hair of a pixel border into the neighbouring pixel, and may order
two nearly equidistant points the other way.  delta = 3 x the largest difference between the float32 and the float64 evaluation of the
fractional pixel coordinates over the case's cloud and poses, rho = 3 x the largest relative fp32-vs-fp64 difference of the depth (the
depth_helpers convention: the model's own gap, x 3 — neither is a chosen number).  A point is a BORDER point for a pose when a pixel
coordinate lies within delta of an integer; a pixel is TIED when an entry of its winning pass lies within rho (relative) of the
winner's depth and carries another colour code.  (Two points with identical coordinates have identical depths in every arithmetic: the
slot decides, that is no tie.)  make_decisive drops every border point and the farther point of every tie until nothing is left to
drop.  Caps on a case: at most DROP_CAP of its points dropped; the kept scene has no border point and no tied pixel."""
import types

import numpy as np

from oracle.oracle import PANO_PASSES

BINS, NCODES = 8, 512
BLACK = NCODES                       # the colour "code" of an exactly black point: never counted, distinct from every real code
U = 2.0 ** -24
# pcl_hist_final_kernel: one rounding per quotient, two adds per thread, a 64-lane wave sum (six adds), four wave partials (three adds),
# on values <= 1
INTER_BOUND = 12 * U
DROP_CAP = 0.03
CERT_MARGIN = 1e-3                   # the device's certificate margin in pixels, max(1e-3, 1.5e-6 W): points between delta and this go
                                     # through pcl_bin_kernel's fix-up queue
VARIANTS = ("rows+1", "cols+1", "fold", "farthest", "centre_first", "round", "transparent", "smallest", "no_carry")


def score_bound(nsh, nsw):
    """the bound of a score: a slot's, plus one rounding per slot summed (pcl_hist_score_kernel; partial sums / (nsh nsw) <= 1)"""
    return INTER_BOUND + (nsh - 2) * nsw * U


# ------------------------------------------------------------------------------------------------- projection
def camera_points(xyz, t, ypr, dtype):
    """R (x - t), every operation in `dtype`"""
    from piccolo_amd import synth
    R = synth.rot_from_ypr_np(np.asarray(ypr, np.float64)).astype(dtype)
    return (np.asarray(xyz).astype(dtype) - np.asarray(t).astype(dtype)[None, :]) @ R.T


def project(cam, H, W):
    """(rowf, colf, depth): make_pano's fractional pixel coordinates (utils.py:44-59, 158-162) and |p|, every operation in cam's dtype"""
    f = cam.dtype.type
    px, py, pz = cam[:, 0], cam[:, 1], cam[:, 2]
    theta = np.arctan2(np.sqrt(px * px + py * py), pz + f(1e-6))
    phi = np.arctan2(py, px + f(1e-6)) + f(np.pi)
    gx = f(2) * (f(1) - phi / f(2 * np.pi)) - f(1)
    gy = f(2) * (theta / f(np.pi)) - f(1)
    colf = (gx + f(1)) / f(2) * f(W - 1)
    rowf = (gy + f(1)) / f(2) * f(H - 1)
    depth = np.sqrt(px * px + py * py + pz * pz)
    assert rowf.dtype == colf.dtype == depth.dtype == cam.dtype
    return rowf, colf, depth


def pixels(rowf, colf, H, W):
    """trunc, then clamp (utils.py:165, 173-188): no wrap at the seam"""
    return np.clip(np.trunc(rowf).astype(np.int64), 0, H - 1), np.clip(np.trunc(colf).astype(np.int64), 0, W - 1)


def color_codes(rgb, rounding=False):
    """per point / pixel: r + 8 g + 64 b of trunc(fp32(rgb) * fp32(255)) // 32 (oracle/hist.py::_codes: the product in float32); BLACK
    where all three products are 0"""
    v = np.asarray(rgb, np.float32) * np.float32(255)
    q = (np.rint(v) if rounding else np.floor(v)).astype(np.int64) // 32
    code = q[..., 0] + BINS * q[..., 1] + BINS * BINS * q[..., 2]
    return np.where((v == 0).all(axis=-1), BLACK, code)


# ------------------------------------------------------------------------------------------------- winners
def resolve(row, col, depth, H, W, keep=None, farthest=False, centre_first=False, smallest=False):
    """-> (winner (H * W,): the point that owns each pixel, -1 where none; entries): latest pass, then nearest, then largest index.
    entries = (pixel, point, first) of every write of a pixel's winning pass, sorted by that priority (first: the winner's entry)."""
    idx = np.arange(len(row)) if keep is None else np.nonzero(keep)[0]
    r, c = row[idx], col[idx]
    passes = list(PANO_PASSES)
    if centre_first:
        passes = passes[8:] + passes[:8]
    last = np.full(H * W, -1, np.int8)
    pix = []
    for p, (dr, dc) in enumerate(passes):
        q = np.clip(r + dr, 0, H - 1) * W + np.clip(c + dc, 0, W - 1)
        pix.append(q)
        last[q] = p
    sel = [last[pix[p]] == p for p in range(9)]
    e_pix = np.concatenate([pix[p][sel[p]] for p in range(9)])
    e_pt = np.concatenate([idx[sel[p]] for p in range(9)])
    d = depth[e_pt]
    o = np.lexsort((e_pt if smallest else -e_pt, -d if farthest else d, e_pix))
    e_pix, e_pt = e_pix[o], e_pt[o]
    first = np.r_[True, e_pix[1:] != e_pix[:-1]] if len(e_pix) else np.zeros(0, bool)
    winner = np.full(H * W, -1, np.int64)
    winner[e_pix[first]] = e_pt[first]
    return winner, (e_pix, e_pt, first)


def tied_points(entries, depth, code, uid, rho, by_code=True):
    """the farther point of every tie: entries of a pixel's winning pass within rho (relative) of the winner's depth, with another colour
    code (by_code=False: any), not a copy of the winner's coordinates"""
    e_pix, e_pt, first = entries
    if not len(e_pix):
        return np.zeros(0, np.int64)
    win = e_pt[np.nonzero(first)[0][np.cumsum(first) - 1]]
    tie = ~first & (depth[e_pt] < depth[win] * (1.0 + rho)) & (uid[e_pt] != uid[win])
    if by_code:
        tie &= code[e_pt] != code[win]
    return np.unique(e_pt[tie])


def relevant(rowf, rows):
    """Can the 3 x 3 footprint of a point with row coordinate rowf touch the pixel rows [rows[0], rows[1])?  (With a whole pixel to spare:
    the row coordinate is well conditioned everywhere — its fp32-vs-fp64 gap is asserted to stay below 1e-3 — while the COLUMN of a point
    next to a pole is not: there phi = atan2(py, px) of two vanishing numbers.)  rows None: every point."""
    if rows is None:
        return np.ones(len(rowf), bool)
    return (rowf >= rows[0] - 2) & (rowf < rows[1] + 2)


def make_decisive(xyz, rgb, poses, H, W, by_code=True, rows=None):
    """poses = (trans (B, 3), rot (B, 3)): every pose the scene is rendered from.  rows: the pixel rows [lo, hi) that are read at all (the
    scored block rows of the histogram stage; None: the whole image) — delta and the border test run over the (point, pose) pairs whose
    footprint can reach them; what a point does in rows nobody reads cannot change a count.
    -> namespace(keep: indices of the kept points, n, dropped: the share dropped, delta, rho, border: share of border points,
    tied: points dropped as ties)"""
    trans, rot = poses
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    code = color_codes(rgb)
    uid = np.unique(xyz, axis=0, return_inverse=True)[1].reshape(-1)
    proj, gap_px, gap_d, gap_row = [], 0.0, 0.0, 0.0
    for b in range(len(trans)):
        r64, c64, d64 = project(camera_points(xyz, trans[b], rot[b], np.float64), H, W)
        r32, c32, d32 = project(camera_points(xyz, trans[b], rot[b], np.float32), H, W)
        rel = relevant(r64, rows)
        gap_row = max(gap_row, float(np.abs(r32 - r64).max()))
        if rel.any():
            gap_px = max(gap_px, float(np.abs(r32 - r64)[rel].max()), float(np.abs(c32 - c64)[rel].max()))
        gap_d = max(gap_d, float((np.abs(d32 - d64) / d64).max()))
        proj.append((r64, c64, d64, rel))
    assert gap_row < 1e-3, gap_row
    delta, rho = 3.0 * gap_px, 3.0 * gap_d
    border = np.zeros(n, bool)
    for r, c, _, rel in proj:
        border |= rel & ((np.abs(r - np.rint(r)) < delta) | (np.abs(c - np.rint(c)) < delta))
    keep = ~border
    ntied = 0
    while True:
        tied = []
        for r, c, d, _ in proj:
            row, col = pixels(r, c, H, W)
            _, ent = resolve(row, col, d, H, W, keep=keep)
            tied.append(tied_points(ent, d, code, uid, rho, by_code))
        tied = np.unique(np.concatenate(tied))
        if not len(tied):
            break
        keep[tied] = False
        ntied += len(tied)
    return types.SimpleNamespace(keep=np.nonzero(keep)[0], n=n, dropped=1.0 - keep.sum() / n, delta=delta, rho=rho, border=float(border.mean()),
                                 tied=ntied)


def undecided(xyz, rgb, poses, H, W, delta, rho, by_code=True, rows=None):
    """(border points, tied points) left in a scene, over all its poses — both must be empty for a decisive one"""
    trans, rot = poses
    code = color_codes(rgb)
    uid = np.unique(np.asarray(xyz, np.float32), axis=0, return_inverse=True)[1].reshape(-1)
    nb, tied = np.zeros(len(xyz), bool), []
    for b in range(len(trans)):
        r, c, d = project(camera_points(xyz, trans[b], rot[b], np.float64), H, W)
        nb |= relevant(r, rows) & ((np.abs(r - np.rint(r)) < delta) | (np.abs(c - np.rint(c)) < delta))
        row, col = pixels(r, c, H, W)
        tied.append(tied_points(resolve(row, col, d, H, W)[1], d, code, uid, rho, by_code))
    return np.nonzero(nb)[0], np.unique(np.concatenate(tied))


def near_integer(xyz, poses, H, W, lo, hi, rows=None):
    """how many (point, pose) pairs (that can reach `rows`) have a pixel coordinate at a distance in [lo, hi) from an integer"""
    trans, rot = poses
    k = 0
    for b in range(len(trans)):
        r, c, _ = project(camera_points(xyz, trans[b], rot[b], np.float64), H, W)
        dist = np.minimum(np.abs(r - np.rint(r)), np.abs(c - np.rint(c)))
        k += int((relevant(r, rows) & (dist >= lo) & (dist < hi)).sum())
    return k


# ------------------------------------------------------------------------------------------------- render, histograms, scores
def render(xyz, rgb, t, ypr, H, W, dtype=np.float64, **how):
    """winner map (H * W,) of one pose"""
    rowf, colf, depth = project(camera_points(xyz, t, ypr, dtype), H, W)
    row, col = pixels(rowf, colf, H, W)
    return resolve(row, col, depth, H, W, **how)[0]


def render_image(xyz, rgb, t, ypr, H, W):
    """the query image a camera at (t, ypr) sees, as a decoded 8-bit file divided by 255 on the host: (H, W, 3) float32"""
    win = render(xyz, rgb, t, ypr, H, W)
    v = np.asarray(rgb, np.float32) * np.float32(255)
    img = np.zeros((H * W, 3), np.uint8)
    img[win >= 0] = np.floor(v[win[win >= 0]]).astype(np.uint8)
    return (img.astype(np.float32) / np.float32(255)).reshape(H, W, 3)


def block_of(H, W, nsh, nsw, variant=None):
    """(H * W,) index of the scored block (h - 1) * nsw + w of every pixel, -1 where it belongs to none"""
    bh, bw = H // nsh, W // nsw
    r, c = np.divmod(np.arange(H * W), W)
    if variant == "rows+1":
        r = r - 1
    if variant == "cols+1":
        c = c - 1
    h, w = np.floor_divide(r, bh), np.floor_divide(c, bw)
    if variant == "fold":
        h, w = np.minimum(h, nsh - 1), np.minimum(w, nsw - 1)
    ok = (h >= 1) & (h <= nsh - 2) & (w >= 0) & (w < nsw)
    return np.where(ok, (h - 1) * nsw + w, -1)


def slot_rule(inter, nproj, nimg, nsh, nsw, carry=True):
    """utils.py:539, 556-580: ONE slot vector for all candidates; an empty block writes 0 and leaves its row, the rest of the row keeps the
    previous candidate's slots.  -> slots (K, nsh * nsw) after each candidate"""
    K = len(inter)
    out, slots = np.zeros((K, nsh * nsw)), np.zeros(nsh * nsw)
    for i in range(K):
        if not carry:
            slots[:] = 0.0
        for h in range(1, nsh - 1):
            for w in range(nsw):
                j = (h - 1) * nsw + w
                if nproj[i, j] == 0 or nimg[j] == 0:
                    slots[h * nsw + w] = 0.0
                    break
                slots[h * nsw + w] = inter[i, j]
        slots[np.isnan(slots)] = 0.0
        out[i] = slots
    return out


def model(xyz, rgb, img, trans, rot, nsh, nsw, dtype=np.float64, variant=None):
    """xyz, rgb: the points in PACKED order; img (H, W, 3) float32; trans, rot (K, 3).  -> namespace(winner (K, H * W), hist (K, nblk, 512),
    hist_q (nblk, 512), nproj (K, nblk), nimg (nblk,), inter (K, nblk), slots (K, nsh * nsw), score (K,))"""
    assert variant is None or variant in VARIANTS
    H, W = int(img.shape[0]), int(img.shape[1])
    K, nblk = len(trans), (nsh - 2) * nsw
    rounding = variant == "round"
    code = color_codes(rgb, rounding)
    blk = block_of(H, W, nsh, nsw, variant)
    img = np.asarray(img, np.float32).reshape(H * W, 3)
    qcode = color_codes(img, rounding)
    qmask = ~(img == 0).all(axis=1)
    assert np.array_equal(qmask, qcode != BLACK)
    how = dict(farthest=variant == "farthest", centre_first=variant == "centre_first", smallest=variant == "smallest")
    if variant == "transparent":
        how["keep"] = code != BLACK

    def hists(mask, codes):
        m = mask & (blk >= 0)
        return np.bincount(blk[m] * NCODES + codes[m], minlength=nblk * NCODES).reshape(nblk, NCODES)

    out = types.SimpleNamespace(hist_q=hists(qmask, qcode), winner=np.empty((K, H * W), np.int64), hist=np.empty((K, nblk, NCODES), np.int64))
    for i in range(K):
        win = render(xyz, rgb, trans[i], rot[i], H, W, dtype, **how)
        wcode = np.where(win >= 0, code[np.maximum(win, 0)], BLACK)
        out.winner[i] = win
        out.hist[i] = hists(qmask & (wcode != BLACK), wcode)
    out.nproj, out.nimg = out.hist.sum(axis=2), out.hist_q.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        hn = out.hist / out.nproj[:, :, None].astype(np.float64)
        qn = out.hist_q / out.nimg[:, None].astype(np.float64)
        inter = np.minimum(hn, qn[None]).sum(axis=2)
    out.inter = np.where((out.nproj == 0) | (out.nimg[None] == 0), 0.0, inter)
    out.slots = slot_rule(out.inter, out.nproj, out.nimg, nsh, nsw, carry=variant != "no_carry")
    out.score = out.slots.sum(axis=1) / (nsh * nsw)
    out.wcode = lambda i: np.where(out.winner[i] >= 0, code[np.maximum(out.winner[i], 0)], BLACK)       # noqa: E731
    return out


def ranking(score, n):
    """flip(argsort()[-n:]) (utils.py:583-586): best first"""
    return np.argsort(score, kind="stable")[-n:][::-1]


def separated(score, n, gap):
    """are the best n scores further than `gap` from each other and from the rest?"""
    s = np.sort(score)[::-1][:n + 1]
    return len(s) < 2 or bool((s[:-1] - s[1:] > gap).all())


def scatter_min_model(cam, H, W):
    """torch_scatter-style scatter-min of |p| over make_pano's centre pixels: (zmin (H * W,) float64, 0 where empty; arg, n where empty;
    smallest index on equal depths)"""
    rowf, colf, d = project(np.asarray(cam, np.float64), H, W)
    row, col = pixels(rowf, colf, H, W)
    pix = row * W + col
    o = np.lexsort((np.arange(len(d)), d, pix))
    first = np.r_[True, pix[o][1:] != pix[o][:-1]]
    zmin, arg = np.zeros(H * W), np.full(H * W, len(d), np.int64)
    zmin[pix[o][first]], arg[pix[o][first]] = d[o][first], o[first]
    return zmin, arg


# ------------------------------------------------------------------------------------------------- the cases
# name -> points of the scene (R6: exactly), panorama, split, candidates, what the shape reaches
CASES = {
    "R1": dict(n=3000, H=63, W=129, nsh=3, nsw=2, K=9),      # image smaller than one tile row, one scored block row, r / bh mapping, fix-up range
    "R2": dict(n=20000, H=130, W=257, nsh=8, nsw=5, K=9),    # bh = 16 < 64, 2-pixel ragged remainder both ways, > 2 x 2 blocks per tile
    "R3": dict(n=60000, H=200, W=330, nsh=5, nsw=3, K=9),    # bw = 110 >= 64 with bh = 40 < 64, tiles cut right and bottom, 30 bin blocks
    "R4": dict(n=40000, H=256, W=512, nsh=4, nsw=4, K=9),    # bh = bw >= 64: big_blocks mapping and the LDS 2 x 2 shortcut
    "R5": dict(n=100, H=40, W=50, nsh=3, nsw=1, K=9),        # fewer points than a bin block, one block column
    "R6a": dict(n=2049, H=64, W=128, nsh=4, nsw=4, K=9, exact=True),     # bin-block boundary + 1
    "R6b": dict(n=4096, H=64, W=128, nsh=4, nsw=4, K=9, exact=True),     # two full bin blocks
    "R7": dict(n=5000, H=65, W=127, nsh=4, nsw=4, K=1),      # one candidate, odd sizes
}
SEED = 90
# Every room carries the same appendix (`appendix`): exact copies of points with other colour codes, a black patch in front of a wall,
# stacks of points per centre pixel and a column of points next to the seam.  The special clouds, each on R1's shape (3 000 points, 63 x 129, 3 x 2), append more or take away:
R1 = dict(n=3000, H=63, W=129, nsh=3, nsw=2)
BASE = ("dup", "black", "stack", "seam")
CASES.update({
    "poles": dict(R1, K=4, kinds=BASE + ("poles",)),         # straight up / down and on the seam: clamped footprints at the image's edges
    "levels": dict(R1, K=9, kinds=BASE + ("levels",)),       # colours on the code edges k / 255, the same levels in the query image
    "empty": dict(R1, K=9, kinds=("seam",), partial=True),   # scored blocks empty for some candidates: the carry-over (batch 16, 5, 1)
})
ROOMS = ("R1", "R2", "R3", "R4", "R5", "R6a", "R6b", "R7")


def reachable(case, variant):
    """Can the shape of `case` tell `variant` from the rule at all?  fold: only a ragged COLUMN remainder lands in a scored block (a
    folded row remainder joins block row nsh - 1, which is not scored); the carry-over needs a second block in a row and a second
    candidate.  Everything else must show in every case."""
    k = CASES[case]
    if variant == "fold":
        return k["W"] % k["nsw"] != 0
    if variant in ("transparent", "smallest"):
        return {"transparent": "black", "smallest": "dup"}[variant] in k.get("kinds", BASE)
    if variant == "no_carry":
        return bool(k.get("partial"))      # (a closed room leaves hardly a scored block empty: the carry-over has a scene of its own)
    return True


def world_points(cam_pts, t, ypr):
    """x = R^T p + t for camera-frame points p of pose (t, ypr), float32"""
    from piccolo_amd import synth
    R = synth.rot_from_ypr_np(np.asarray(ypr, np.float64))
    return (np.asarray(cam_pts, np.float64) @ R + np.asarray(t, np.float64)[None, :]).astype(np.float32)


def direction(az, el):
    """unit camera-frame vector at azimuth az, elevation el above the horizon (the horizon is the panorama's middle row)"""
    return np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])


def patch(rng, t, ypr, az, el, dist, size, count):
    """`count` world points on a square of `size` metres facing the camera at (t, ypr), `dist` metres away in direction (az, el)"""
    d = direction(az, el)
    e1 = np.cross(d, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    uv = rng.uniform(-size / 2, size / 2, size=(count, 2))
    return world_points(dist * d[None] + uv[:, :1] * e1[None] + uv[:, 1:] * e2[None], t, ypr)


def appendix(rng, room_xyz, room_rgb, gt, poses, n, kinds, H, W):
    """The points every case carries next to its room, built on purpose (each kind a few per cent of n at the most):
    dup     exact copies of room points with the complementary colour (another code): the largest packed slot wins
    black   a patch of exactly black points 0.9 m in front of the query camera: hides the wall, renders nothing
    stack   several points per centre pixel of candidates 0 and 1 at distinct depths, consecutive in the input: pre-dedup food
    seam    a column of points half a pixel off the seam of the query camera and of candidate 0, over the scored rows: the last image column
            (only clamped footprints reach it) is painted in the query and in a render
    levels  a patch whose colours sit on the code edges k / 255
    poles   points just off straight up / straight down and just off the seam of the first candidates: clamped footprints"""
    t_gt, ypr_gt = gt
    trans, rot = poses
    xs, cs = [], []
    if "dup" in kinds:
        pick = rng.choice(len(room_xyz) // 2, size=max(4, n // 50), replace=False)
        xs.append(room_xyz[pick])
        cs.append((1.0 - room_rgb[pick]).astype(np.float32))
    if "black" in kinds:
        k = max(12, n // 40)
        xs.append(patch(rng, t_gt, ypr_gt, 0.7, 0.05, 0.9, 0.5, k))
        cs.append(np.zeros((k, 3), np.float32))
    if "stack" in kinds:
        for b in range(min(2, len(trans))):
            for _ in range(max(2, n // 400)):
                d = direction(rng.uniform(0, 2 * np.pi), rng.uniform(-0.3, 0.3))
                dist = 0.5 + 0.07 * np.arange(4)
                xs.append(world_points(dist[:, None] * d[None], trans[b], rot[b]))
                cs.append(rng.uniform(0.05, 0.95, size=(4, 3)).astype(np.float32))
    if "seam" in kinds:
        ph = 0.5 * 2 * np.pi / (W - 1)                                   # column coordinate W - 1.5
        for t, ypr in ((t_gt, ypr_gt), (trans[0], rot[0])):
            els = np.linspace(-0.45, 0.45, max(6, min(24, n // 100)))
            xs.append(world_points(np.stack([-np.cos(ph) * np.cos(els), -np.sin(ph) * np.cos(els), np.sin(els)], axis=1), t, ypr))
            cs.append(rng.uniform(0.05, 0.95, size=(len(els), 3)).astype(np.float32))
    if "levels" in kinds:
        lv = np.array([31, 32, 33, 63, 64, 223, 224, 255], np.float32) / np.float32(255)
        k = max(64, n // 20)
        xs.append(patch(rng, t_gt, ypr_gt, 2.5, -0.05, 0.8, 0.6, k))
        cs.append(lv[rng.integers(0, len(lv), size=(k, 3))])
    if "poles" in kinds:
        for b in range(len(trans)):
            pts = []
            for frac in (0.3, 0.6):
                th = frac * np.pi / (H - 1)                              # row coordinate `frac` below the top / above the bottom
                for az in (0.4, 2.0, 3.9):
                    pts.append(1.1 * np.array([np.sin(th) * np.cos(az), np.sin(th) * np.sin(az), np.cos(th)]))
                    pts.append(1.1 * np.array([np.sin(th) * np.cos(az), np.sin(th) * np.sin(az), -np.cos(th)]))
                ph = frac * 2 * np.pi / (W - 1)                          # column coordinate W - 1 - frac / frac: either side of the seam
                for el in (-0.2, 0.0, 0.25):
                    pts.append(1.0 * np.array([-np.cos(ph) * np.cos(el), -np.sin(ph) * np.cos(el), np.sin(el)]))
                    pts.append(1.0 * np.array([-np.cos(ph) * np.cos(el), np.sin(ph) * np.cos(el), np.sin(el)]))
            xs.append(world_points(np.array(pts), trans[b], rot[b]))
            cs.append(rng.uniform(0.05, 0.95, size=(len(pts), 3)).astype(np.float32))
    if not xs:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    return np.concatenate(xs).astype(np.float32), np.concatenate(cs).astype(np.float32)


def scored_rows(H, nsh):
    return (H // nsh, (nsh - 1) * (H // nsh))


def build_scene(n, H, W, K, nsh, seed=SEED, kinds=BASE, exact=False, partial=False, gts=1, by_code=True, recolor=False, **_):
    """A decisive scene of about n points (exact: exactly n): a box room with its appendix, `gts` query poses with K candidates each,
    start_poses(sigma_t=0.5, sigma_r=0.4).  partial: only the room's +x wall and the half of the floor in front of it, the query camera facing it (the wall on either side of the
    panorama's middle column) and candidate i turned a further i / K of a full turn: the wall passes through every block column and leaves
    the others empty.  recolor: a second colouring per further image (colour sets; ties are then decided without looking at the codes).
    -> namespace(xyz, rgb, rgbs, gt, poses, trans (gts, K, 3), rot, imgs (gts of (H, W, 3)), imgs_sets (image g in colouring g), H, W, rows,
    by_code, info: make_decisive's report)"""
    from piccolo_amd import synth
    rng = np.random.default_rng(seed)
    pool_xyz, pool_rgb = synth.box_room((int(n * 1.5) + 64) * (12 if partial else 1), seed)
    if partial:
        m = (pool_xyz[:, 0] == pool_xyz[:, 0].max()) | ((pool_xyz[:, 2] == pool_xyz[:, 2].min()) & (pool_xyz[:, 0] > 0.0))
        pool_xyz, pool_rgb = pool_xyz[m], pool_rgb[m]
    gt_t, gt_r, trans, rot = [], [], [], []
    for g in range(gts):
        t_gt, ypr_gt = synth.gt_pose(seed + g)
        if partial:
            ypr_gt[0] = 0.05
        tr, ro = synth.start_poses(t_gt, ypr_gt, K, seed=seed + g, sigma_t=0.5, sigma_r=0.4)
        if partial:
            ro[:, 0] = ypr_gt[0] - (2 * np.pi * np.arange(K) / K).astype(np.float32)
        gt_t.append(t_gt), gt_r.append(ypr_gt), trans.append(tr), rot.append(ro)
    # (the query image is an INPUT, rendered below by the model itself: its own pose needs no decision)
    poses, rows = (np.concatenate(trans), np.concatenate(rot)), scored_rows(H, nsh)
    ax, ac = appendix(rng, pool_xyz[:n], pool_rgb[:n], (gt_t[0], gt_r[0]), (trans[0], rot[0]), n, kinds, H, W)
    m = n - len(ax)
    assert 0 < m, "the appendix is larger than the case"
    for _ in range(16):
        assert m <= len(pool_xyz)
        xyz, rgb = np.concatenate([pool_xyz[:m], ax]), np.concatenate([pool_rgb[:m], ac])
        info = make_decisive(xyz, rgb, poses, H, W, by_code and not recolor, rows)
        if not exact or len(info.keep) == n:
            break
        m += n - len(info.keep)
    else:
        raise AssertionError("no cloud of exactly %d decisive points" % n)
    xyz, rgb = np.ascontiguousarray(xyz[info.keep]), np.ascontiguousarray(rgb[info.keep])
    rgbs = [rgb]
    if recolor:
        rgbs = [rgb] + [np.ascontiguousarray(np.roll(rgb, g, axis=1) * np.float32(1.0 - 0.1 * g)) for g in range(1, gts)]
    imgs = [render_image(xyz, rgb, gt_t[g], gt_r[g], H, W) for g in range(gts)]
    imgs_sets = [render_image(xyz, rgbs[g], gt_t[g], gt_r[g], H, W) for g in range(gts)] if recolor else imgs
    if "levels" in kinds:
        imgs = [stamp_levels(im, nsh) for im in imgs]
    return types.SimpleNamespace(xyz=xyz, rgb=rgb, rgbs=rgbs, gt=(np.stack(gt_t), np.stack(gt_r)), poses=poses, trans=np.stack(trans), rot=np.stack(rot),
                                 imgs=imgs, imgs_sets=imgs_sets, H=H, W=W, rows=rows, by_code=by_code and not recolor, info=info)


def camera_scene(n, H, W, seed=SEED, **_):
    """A decisive CAMERA-FRAME cloud for the stand-alone make_pano / scatter-min (every pixel is read, ties are decided without looking at
    the colours): the room as the query camera sees it, with copies of points, a black patch, points just off the poles and the seam.
    The pose of the model is the identity."""
    from piccolo_amd import synth
    rng = np.random.default_rng(seed + 1000)
    xyz, rgb = synth.box_room(n, seed)
    t_gt, ypr_gt = synth.gt_pose(seed)
    ident = (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    cam = synth.transform_cloud(xyz, t_gt, ypr_gt)
    ax, ac = appendix(rng, cam, rgb, (ident[0][0], ident[1][0]), ident, n, ("dup", "black", "poles"), H, W)
    cam, rgb = np.concatenate([cam, ax]), np.concatenate([rgb, ac])
    info = make_decisive(cam, rgb, ident, H, W, by_code=False)
    return types.SimpleNamespace(xyz=np.ascontiguousarray(cam[info.keep]), rgb=np.ascontiguousarray(rgb[info.keep]), poses=ident, H=H, W=W, rows=None,
                                 by_code=False, info=info)


def stamp_levels(img, nsh):
    """the colour levels on the code edges in the query image too: an 8 x 8 patch in the first scored block row"""
    lv = np.array([31, 32, 33, 63, 64, 223, 224, 255], np.float32) / np.float32(255)
    r0 = img.shape[0] // nsh + 1
    out = img.copy()
    for k in range(8):
        out[r0:r0 + 8, 2 + k, 0] = lv[k]
        out[r0 + k, 2:10, 1] = lv[k]
        out[r0:r0 + 8, 2 + k, 2] = lv[(k + 3) % 8]
    return out
