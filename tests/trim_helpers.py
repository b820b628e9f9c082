"""The trim kernel, pair by pair (not a test module; tests/test_trim_points.py).

A cloud of ONE point x under K translations and a table of R rotations is K x R (point, pose) pairs: the kernel only sees x - t_k, so entry
[k, r] of trim_loss_table is that pair's own ||c - rgb|| (NaN, count 0, where the sample is exact black).  The model is
grad_helpers.model over tt = repeat(trans, R), rr = tile(rot, K) in float64 and float32; grad_helpers.decisive says which pairs can be
compared.  One class is the trim kernel's own, the SEAM pair: p_x < 0 and a p_y whose sign the two models do not share, or that is no
larger than 3 x their difference.  Which end of the panorama such a pair lands on is decided by a p_y of 1e-8; the kernel's contract
there is the generic forward kernel's end, not float64's.

emulate(): the kernel's OWN arithmetic restated in float64 — q' = M (x - t) under the class's first rotation, phi0, the member's yaw, the
first-order carry of the reference's x + 1e-6, the exact branch inside `tiny`, the first-order correction of a member whose third row is not
the first rotation's, the sign of p_y at the seam — with the planted mistakes of VARIANTS, to show that the comparison would notice them."""
import numpy as np

import grad_helpers as gh

EPS = gh.EPS
TOL = 4e-7                  # third rows equal to this: one class (csrc/pcl_trim.hip)
NY = 4                      # yaws per sub-group
TINY_OLD = 1e-8             # rho^2 below which the kernel took the exact arctangent before this comparison existed
# The carry phi = phi0 + delta - eps p_y / rho^2 drops (eps / rho)^2 / 2 rad = (eps / rho)^2 / (4 pi) turns.  That must stay below half an
# ulp of the fp32 column coordinate in turns (values in [0.25, 0.5): ulp 2^-24, half of it 2^-25): rho^2 >= eps^2 2^25 / (4 pi) = 2.67e-6
TINY = 2.7e-6
SEAM = 0.49999
MERGE_CONE = 0.1            # rad from the vertical axis within which a member of a merged class gets its first-order correction
POINT, RGB = gh.POINT, np.array([0.3, 0.6, 0.9], np.float32)
FLOAT_SCALE = np.float32(0.9173)          # the float image of a case: its k/255 image times this (not k/255)

VARIANTS = {
    "no_carry": "(a) the carry dropped: phi0 + delta",
    "first_order": "(b) the carry kept to first order only outside rho^2 < 1e-8",
    "seam_sum": "(c) the seam end taken from the sign of the summed angle",
    "pair_row": "(d) the second row of an odd-row footprint taken from the same element row (U8P pairing)",
    "rot_idx": "(e) the entries of a class rotated by one member",
    "padded_slot": "(f) a padded slot of a short sub-group written to the table",
    "black_tap": "(g) a footprint with one black tap masked",
    "merged_row": "(h) a member of a merged class evaluated with the third row of the class's first rotation",
}


# ------------------------------------------------------------------------------------------------------------ rotation tables
def _matrix(ypr):
    from piccolo_amd import synth
    return synth.rot_from_ypr_np(np.asarray(ypr, np.float64))


def stanford24():
    """the 24 distinct rotations of the 4 x 4 x 4 grid of quarter turns (fp32 roundings of k pi / 2), in first-occurrence order"""
    q = (np.arange(4, dtype=np.float32) / np.float32(4)) * np.float32(2 * np.pi)
    keep, seen = [], []
    for y in q:
        for p in q:
            for r in q:
                M = np.round(_matrix([y, p, r]))
                if not any(np.array_equal(M, s) for s in seen):
                    seen.append(M)
                    keep.append([y, p, r])
    return np.array(keep, np.float32)


def yaw8():
    rot = np.zeros((8, 3), np.float32)
    rot[:, 0] = np.arange(8) * 2 * np.pi / 8
    return rot


def ragged():
    """classes of 5, 3, 2 and 1 members, interleaved; yaws outside [0, 2 pi); the class of 2 is two rotations whose pitch differs by one
    fp32 ulp (third rows 1.2e-7 apart: merged), the class of 1 is 16 ulps further (1.8e-6 apart: not merged)"""
    a, b = (0.3, -0.4), (-0.6, 0.9)
    p0 = np.float32(1.2)
    p1, p2 = np.nextafter(p0, np.float32(2)), p0 + 17 * np.spacing(p0)
    rows = [(0.7,) + a, (2.5,) + b, (-2.9,) + a, (0.4, p0, 2.8), (7.5,) + a, (-4.1,) + b, (1.9, p1, 2.8), (1.1,) + a, (9.0,) + b,
            (-0.8, p2, 2.8), (-12.0,) + a]
    return np.array(rows, np.float32)


RAGGED_SIZES = [5, 3, 2, 1]
_TABLES = {"stanford": stanford24, "yaw8": yaw8, "ragged": ragged}
TABLES = tuple(_TABLES)
_CACHE = {}


def table(name):
    if ("table", name) not in _CACHE:
        _CACHE["table", name] = _TABLES[name]()
    return _CACHE["table", name]


def classes(rot):
    """what pcl_trim_groups_kernel finds, in float64 on the host: leader (R,), the member's yaw relative to it delta (R,), and the
    sub-groups [(leader, [members])] of at most NY members in the order of the classes' first rotations"""
    rot = np.asarray(rot, np.float32)
    M = np.stack([_matrix(r) for r in rot])
    R = len(rot)
    leader = np.arange(R)
    for r in range(R):
        for j in range(r):
            if leader[j] == j and np.abs(M[j, 2] - M[r, 2]).max() <= TOL:
                leader[r] = j
                break
    delta = np.array([np.arctan2(M[r, 1] @ M[leader[r], 0], M[r, 0] @ M[leader[r], 0]) if leader[r] != r else 0.0 for r in range(R)])
    groups = []
    for l in range(R):
        if leader[l] == l:
            mem = [r for r in range(R) if leader[r] == l]
            groups += [(l, mem[i:i + NY]) for i in range(0, len(mem), NY)]
    return dict(leader=leader, delta=delta, groups=groups, M=M, sizes=[int((leader == l).sum()) for l in range(R) if leader[l] == l])


# ------------------------------------------------------------------------------------------------------------------ panoramas
PANOS = {"lv64": (64, 128), "lv16": (16, 32), "lv300": (300, 100), "lv127": (127, 250), "lv1024": (1024, 2048)}


def levels_pano(H, W, seed=0):
    """random levels 1..255 with six black rectangles, k/255 in float32"""
    rng = np.random.default_rng(1000 * H + W + seed)
    lev = rng.integers(1, 256, size=(H, W, 3))
    for _ in range(6):
        h, w = int(rng.integers(max(H // 25, 1), H // 5 + 2)), int(rng.integers(max(W // 25, 1), W // 6 + 2))
        y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
        lev[y:y + h, x:x + w] = 0
    return lev.astype(np.float32) / 255


# ------------------------------------------------------------------------------------------------------------- translation sets
RHOS = (1.05e-4, 2e-4, 3e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2, 5e-5)     # the last one is inside the old `tiny`
N_AZIMUTH = 40
N_RANDOM = 300
PROBE_SETS = ("seam", "poles", "border16", "border300", "fractions", "black", "rho", "axis")


def aimed_translations(x, targets, rot):
    """every target (gx, gy, rho) aimed at every rotation of the table: t = x - R^T aim(...), float32 -> trans (len(rot) * m, 3),
    aimed (K, R) bool: pair [k, r] is the one translation k was made for"""
    tg = np.asarray(targets, np.float64).reshape(-1, 3)
    p = gh.aim(tg[:, 0], tg[:, 1], tg[:, 2])
    trans = np.concatenate([np.asarray(x, np.float64)[None, :] - p @ _matrix(r) for r in rot]).astype(np.float32)
    aimed = np.zeros((len(trans), len(rot)), bool)
    for j in range(len(rot)):
        aimed[j * len(p):(j + 1) * len(p), j] = True
    return trans, aimed


def exact_seam_translations(x, rot):
    """q_y = q_z = 0 and p_x < 0 under a rotation of the table: t = x - R^T (-d, 0, 0); the seam branch then decides from a p_y that is
    rounding dust.  Distinct translations only (the quarter turns give six per distance)."""
    out = []
    for d in (1.0, 3.0):
        for r in rot:
            t = (np.asarray(x, np.float64) - np.array([-d, 0.0, 0.0]) @ _matrix(r)).astype(np.float32)
            if not any(np.array_equal(t, o) for o in out):
                out.append(t)
    return np.array(out, np.float32)


def near_axis_translations():
    """the point at the origin, |t| of the order of rho: horizontal distance rho at N_AZIMUTH azimuths, height within +-0.8 rho"""
    rng = np.random.default_rng(5)
    out = []
    for rho in RHOS:
        az = (np.arange(N_AZIMUTH) + rng.random(N_AZIMUTH)) * 2 * np.pi / N_AZIMUTH
        out.append(-np.stack([rho * np.cos(az), rho * np.sin(az), rho * rng.uniform(-0.8, 0.8, N_AZIMUTH)], 1))
    return np.concatenate(out).astype(np.float32)


def one_point_cases():
    """[(set, panorama, table)]: every one-point case of section 3"""
    out = []
    for tb in TABLES:
        out += [(s, "probe", tb) for s in PROBE_SETS] + [("poles", "lv127", tb)]
        out += [("random", p, tb) for p in PANOS]
    out += [("near_axis", p, tb) for p in ("lv64", "lv1024") for tb in ("stanford", "yaw8")]
    return out


def case_id(c):
    return "-".join(c)


def case(c):
    """-> dict(x, rgb, img (k/255), imgf (float, not k/255), trans (K,3), rot (R,3), aimed (K,R) bool), computed once"""
    if ("case", c) in _CACHE:
        return _CACHE["case", c]
    name, pano, tb = c
    rot = table(tb)
    x, rgb, aimed = POINT, RGB, None
    if pano != "probe":
        if ("pano", pano) not in _CACHE:
            _CACHE["pano", pano] = levels_pano(*PANOS[pano])
        img = _CACHE["pano", pano]
    if name in PROBE_SETS:
        k = gh.probe_targets(name)
        x, rgb = k["x"], k["rgb"]
        if pano == "probe":
            img = k["img"]
        trans, aimed = aimed_translations(x, k["targets"], rot)
        if name == "seam":
            extra = exact_seam_translations(x, rot)
            trans = np.concatenate([trans, extra])
            aimed = np.concatenate([aimed, np.zeros((len(extra), len(rot)), bool)])
    elif name == "random":
        trans = np.random.default_rng(PANOS[pano][1]).uniform(-1.5, 1.5, size=(N_RANDOM, 3)).astype(np.float32)
    elif name == "near_axis":
        x, trans = np.zeros(3, np.float32), near_axis_translations()
    else:
        raise KeyError(name)
    if aimed is None:
        aimed = np.zeros((len(trans), len(rot)), bool)
    _CACHE["case", c] = dict(x=x, rgb=rgb, img=img, imgf=(img * FLOAT_SCALE).astype(np.float32), trans=trans, rot=rot, aimed=aimed)
    return _CACHE["case", c]


def pairs(trans, rot):
    """row-major (K, R) like the table"""
    return np.repeat(trans, len(rot), 0), np.tile(rot, (len(trans), 1))


# ------------------------------------------------------------------------------------------------------- the model and the rule
def seam_pairs(m64, m32):
    p64, p32 = m64["p"], m32["p"].astype(np.float64)
    y64, y32 = p64[:, 1], p32[:, 1]
    return (p64[:, 0] < 0) & ((np.signbit(y64) != np.signbit(y32)) | (np.abs(y64) <= 3 * np.abs(y32 - y64)))


def rule_of(m64, m32):
    """the slim record of a pair of models: loss64, loss32, kept, ok (decisive and no seam pair), seam, seam_ok (a seam pair whose ROW
    and mask are decisive: it goes to the generic kernel), rho (distance from the camera's vertical axis), x0 / y0 (footprint start)"""
    seam = seam_pairs(m64, m32)
    # (a seam pair's two models sit W px apart: it must not set the case's gap)
    rest = [{key: (v[~seam] if isinstance(v, np.ndarray) else v) for key, v in m.items()} for m in (m64, m32)]
    ok = np.zeros(len(seam), bool)
    ok[~seam], delta, gap = gh.decisive(*rest)
    H = m64["H"]
    iy = m64["iy"]
    p = m64["p"]
    rho, r = np.hypot(p[:, 0], p[:, 1]), np.sqrt((p * p).sum(1))
    row_ok = (rho >= gh.CONE * r) & ~(m64["in_y"] & (np.abs(iy - np.round(iy)) < delta)) & (np.abs(np.abs(m64["gy"]) - gh.LIM) * H / 2 >= delta)
    lim = gh.LIM
    cx, cy = np.clip(m64["gx"], -lim, lim), np.clip(m64["gy"], -lim, lim)
    return dict(l64=m64["loss"], l32=m32["loss"].astype(np.float64), kept=m64["kept"], kept32=m32["kept"], ok=ok, seam=seam,
                seam_ok=seam & row_ok, border=~ok & ~seam, rho=rho, delta=delta, gap=gap, py64=p[:, 1], py32=m32["p"][:, 1].astype(np.float64),
                x0=np.floor(((cx + 1) * m64["W"] - 1) / 2).astype(np.int64), y0=np.floor(((cy + 1) * H - 1) / 2).astype(np.int64), H=H, W=m64["W"])


def rule_for(oracle, k, img, rgb=None):
    """the rule of a case's pairs on another image / with another colour of the point"""
    tt, rr = pairs(k["trans"], k["rot"])
    rgb = k["rgb"] if rgb is None else rgb
    m64 = gh.model(oracle, k["x"][None, :], rgb[None, :], img, tt, rr, np.float64)
    m32 = gh.model(oracle, k["x"][None, :], rgb[None, :], img, tt, rr, np.float32)
    return rule_of(m64, m32)


def rule(oracle, c, flt=False):
    """the rule of a case on its k/255 image (flt: on its float image), computed once"""
    if ("rule", c, flt) not in _CACHE:
        k = case(c)
        _CACHE["rule", c, flt] = rule_for(oracle, k, k["imgf"] if flt else k["img"])
    return _CACHE["rule", c, flt]


def errors(out, ref, sel, s=None):
    """|out - ref| / max(ref, s) over the pairs `sel`, s the median of ref there; a NaN or infinity in `out` is an infinite error"""
    out, ref = np.asarray(out, np.float64).reshape(-1)[sel], np.asarray(ref, np.float64).reshape(-1)[sel]
    if len(ref) == 0:
        return np.zeros(0)
    s = max(float(np.median(ref)), 1e-300) if s is None else s
    with np.errstate(invalid="ignore"):
        e = np.abs(out - ref) / np.maximum(ref, s)
    return np.where(np.isfinite(e), e, np.inf)


def yardstick(ru, sel=None):
    sel = (ru["ok"] & ru["kept"]) if sel is None else sel
    return gh.three_stats(errors(ru["l32"], ru["l64"], sel))


def breaks(ru, loss, kept, sel=None):
    """does a (loss, kept) of all pairs break what the device is held to on the decisive pairs `sel` (default: all of them)?"""
    sel = ru["ok"] if sel is None else sel & ru["ok"]
    loss, kept = np.asarray(loss, np.float64).reshape(-1), np.asarray(kept).reshape(-1)
    if not np.array_equal(kept[sel], ru["kept"][sel]):
        return True
    sel = sel & ru["kept"]
    s = max(float(np.median(ru["l64"][ru["ok"] & ru["kept"]])), 1e-300)
    return gh.exceeds(gh.three_stats(errors(loss, ru["l64"], sel, s)), gh.three_stats(errors(ru["l32"], ru["l64"], sel, s)))


# --------------------------------------------------------------------------------------------- the kernel's formula in float64
def sample(img, coord, mode=None):
    """the bilinear sample of the float64 image with its zero border -> (c (m,3), kept (m,)).  mode "pair_row": a footprint that starts
    on an odd row of the bordered texture (an even image row) reads its second row from the element row it started in, i.e. the row
    ABOVE its first; "black_tap": a footprint with a black tap is masked"""
    H, W, _ = img.shape
    g = np.clip(coord, -gh.LIM, gh.LIM)
    ix, iy = ((g[:, 0] + 1) * W - 1) / 2, ((g[:, 1] + 1) * H - 1) / 2
    fx0, fy0 = np.floor(ix), np.floor(iy)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    wx1, wy1 = (ix - fx0)[:, None], (iy - fy0)[:, None]
    wx0, wy0 = 1 - wx1, 1 - wy1

    def tap(y, x):
        v = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return np.where(((x >= 0) & (x < W) & (y >= 0) & (y < H))[:, None], v, 0.0)
    y1 = np.where((y0 + 1) % 2 == 1, y0 - 1, y0 + 1) if mode == "pair_row" else y0 + 1
    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y1, x0), tap(y1, x0 + 1)
    c = v00 * (wx0 * wy0) + v01 * (wx1 * wy0) + v10 * (wx0 * wy1) + v11 * (wx1 * wy1)
    kept = (c != 0).any(1)
    if mode == "black_tap":
        kept &= ~np.stack([(v == 0).all(1) for v in (v00, v01, v10, v11)]).any(0)
    return c, kept


def emulate(oracle, k, img, variant=None, tiny=TINY):
    """(loss, kept) of all K x R pairs of a case by the kernel's own formula in float64, with a planted variant"""
    assert variant is None or variant in VARIANTS, variant
    rot, x = k["rot"], k["x"].astype(np.float64)
    K, R = len(k["trans"]), len(rot)
    cl = classes(rot)
    L, delta, M = cl["leader"], cl["delta"], cl["M"]
    w = x[None, :] - k["trans"].astype(np.float64)                            # (K,3)
    q = np.einsum("rij,kj->kri", M[L], w)                                     # q' = M (x - t) under the class's first rotation
    qx, qy, qz = q[..., 0], q[..., 1], q[..., 2]
    sd, cd = np.sin(delta)[None, :], np.cos(delta)[None, :]
    px, py = cd * qx - sd * qy, sd * qx + cd * qy
    rho2 = qx * qx + qy * qy
    # a member of a merged class: (R_member R_first^T)[0..1][2] q'_z is what its own matrix adds to p_x, p_y near the axis
    ex, ey = np.einsum("rj,rj->r", M[:, 0], M[L, 2]), np.einsum("rj,rj->r", M[:, 1], M[L, 2])
    off = (np.abs(ex) < 1e-12) & (np.abs(ey) < 1e-12) if variant != "merged_row" else np.ones(R, bool)
    ex, ey = np.where(off, 0.0, ex)[None, :], np.where(off, 0.0, ey)[None, :]
    near = np.abs(np.arctan2(qz + EPS, np.sqrt(rho2))) > np.pi / 2 - MERGE_CONE
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.arctan2(qy, qx) + delta[None, :] - (0.0 if variant == "no_carry" else EPS * py / rho2)
        first = first + np.where(near, (px * ey - py * ex) * qz / rho2, 0.0)
    px, py = px + ex * qz, py + ey * qz
    exact = np.arctan2(py, px + EPS)
    phi = np.where(rho2 < (TINY_OLD if variant in ("first_order", "no_carry") else tiny), exact, first)
    u = 0.5 - phi / (2 * np.pi)
    g = (u - np.floor(u)) - 0.5
    if variant != "seam_sum":
        # the sign of p_y from the member's OWN fp32 matrix row, as the generic kernel multiplies it
        row1 = np.stack([oracle.rot_from_ypr(r, np.float32)[1] for r in rot]).astype(np.float32)
        w32 = (k["x"].astype(np.float32)[None, :] - k["trans"].astype(np.float32))
        pye = ((row1[None, :, 0] * w32[:, None, 0] + row1[None, :, 1] * w32[:, None, 1]) + row1[None, :, 2] * w32[:, None, 2]).astype(np.float64)
        g = np.where(np.abs(g) > SEAM, np.where(np.signbit(-pye), -np.abs(g), np.abs(g)), g)
    gy = oracle.cloud2idx(np.stack([px, py, qz], -1).reshape(-1, 3), np.float64)[:, 1]
    coord = np.stack([2 * g.reshape(-1), gy], 1)
    c, kept = sample(np.asarray(img, np.float64), coord, variant if variant in ("pair_row", "black_tap") else None)
    d = c - k["rgb"].astype(np.float64)[None, :]
    loss = np.where(kept, np.sqrt((d * d).sum(1)), np.nan).reshape(K, R)
    kept = kept.reshape(K, R)
    if variant == "rot_idx":
        for l in np.nonzero(L == np.arange(R))[0]:
            mem = np.nonzero(L == l)[0]
            loss[:, mem], kept[:, mem] = loss[:, np.roll(mem, 1)], kept[:, np.roll(mem, 1)]
    if variant == "padded_slot":
        # a padded slot holds yaw 0 relative to the class's first rotation and rot_idx -1: entry k * R - 1 = [k - 1, R - 1]
        for l, mem in cl["groups"]:
            if len(mem) < NY:
                loss[:-1, R - 1], kept[:-1, R - 1] = loss[1:, l], kept[1:, l]
    return loss.reshape(-1), kept.reshape(-1)


# ----------------------------------------------------------------------------------- clouds of distinct points (section 4)
LANE_SIZES = (2, 255, 256, 257, 511, 512, 513, 1025)
LANE_TRANS = np.array([[0.3, -0.2, 0.1], [-1.1, 0.8, -0.4], [1.7, -1.2, 0.6]], np.float32)
LANE_POOL, LANE_SEED = 2048, 23


def lanes(oracle, tb):
    """box_room points of a fixed seed of which EVERY (point, pose) pair under LANE_TRANS x the table is decisive and no seam pair, on
    the 127 x 250 panorama -> dict(xyz, rgb (P,3), l64, l32 (P, K R: NaN where masked), img)"""
    if ("lanes", tb) not in _CACHE:
        from piccolo_amd import synth
        xyz, rgb = synth.box_room(LANE_POOL, seed=LANE_SEED)
        if ("pano", "lv127") not in _CACHE:
            _CACHE["pano", "lv127"] = levels_pano(*PANOS["lv127"])
        img = _CACHE["pano", "lv127"]
        tt, rr = pairs(LANE_TRANS, table(tb))
        good = np.ones(len(xyz), bool)
        l64, l32 = [], []
        for t, r in zip(tt, rr):
            m64, m32 = gh.model(oracle, xyz, rgb, img, t, r, np.float64), gh.model(oracle, xyz, rgb, img, t, r, np.float32)
            ru = rule_of(m64, m32)
            good &= ru["ok"]
            l64.append(ru["l64"])
            l32.append(m32["loss"])
        idx = np.nonzero(good)[0]
        _CACHE["lanes", tb] = dict(xyz=xyz[idx], rgb=rgb[idx], l64=np.stack(l64, 1)[idx], l32=np.stack(l32, 1)[idx].astype(np.float32), img=img,
                                   pool=len(xyz))
    return _CACHE["lanes", tb]


def lane_means(ln, n):
    """of the first n points: count (K R,), the float64 mean of the model's kept terms, and the float32 model's mean (float32 terms,
    summed and divided in float32)"""
    l64, l32 = ln["l64"][:n], ln["l32"][:n]
    kept = ~np.isnan(l64)
    count = kept.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m64 = np.where(kept, l64, 0.0).sum(0) / count
        m32 = np.where(kept, l32, np.float32(0)).sum(0, dtype=np.float32) / count.astype(np.float32)
    return count, m64, m32.astype(np.float64)
