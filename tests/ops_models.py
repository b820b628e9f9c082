"""Plain numpy models of the stand-alone ops (csrc/pcl_ops.hip) and the packers (csrc/pcl_pack.hip): float64 or integer, one rule per
function, no device, no oracle (not a test module; tests/test_ops_exact.py and tests/test_pack_exact.py hold the device to them).

Every model that a planted-mistake test needs takes the mistake as a keyword (all off by default): the CPU tests show that the comparison
the device is held to fails for each of them, so no wrong kernel is ever built or run.

Inputs of the pixel-exact tests are CONSTRUCTED so that no fp32 rounding can move a point across a pixel edge (pano_points: the point sits
at a fraction in [0.25, 0.75] of its pixel) and no contracted x*x + y*y + z*z can reorder two depths (depth levels a factor 1.0011 apart,
or bit-identical rows): winners are then decided by the rule alone and compared with array_equal."""
import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = F64(F32(1e-6))                 # the projection's 1e-6 as the fp32 constant every fp32 evaluation (reference and kernel) adds
LIM32 = F32(0.99)                      # sample_from_img's clip, as fp32 compares it
# make_pano's nine passes in the order they are issued, idx8 .. idx1 then the centre, as (drow, dcol): a later pass overwrites an earlier one
PANO_PASSES = [(0, -1), (0, 1), (-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1), (0, 0)]
DEPTH_RATIO = 1.0011                   # neighbouring depth levels: a relative gap above 1e-3
DEPTH_GAP = 1e-3


# ================================================================================================ projection, pixels
def cloud2idx(xyz, dtype=F64):
    """(n, 2) = (gx, gy) of camera-frame points: theta = atan2(|p_xy|, z + 1e-6), phi = atan2(y, x + 1e-6) + pi,
    g = (2 (1 - phi / 2 pi) - 1, 2 theta / pi - 1), in the operation order of the reference"""
    p = np.asarray(xyz, dtype).reshape(-1, 3)
    eps, pi = dtype(EPS32), dtype(np.pi)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rho = np.sqrt(x * x + y * y)
    theta = np.arctan2(rho, z + eps)
    phi = np.arctan2(y, x + eps) + pi
    cx = dtype(1) - phi / (dtype(2) * pi)
    cy = theta / pi
    return np.stack([dtype(2) * cx - dtype(1), dtype(2) * cy - dtype(1)], 1)


def cloud2idx_backward(xyz, grad_coord, dtype=F64):
    """grad_xyz = J^T grad_coord by the kernel's stated chain rule; the norm's subgradient at rho = 0 is 0"""
    p, G = np.asarray(xyz, dtype).reshape(-1, 3), np.asarray(grad_coord, dtype).reshape(-1, 2)
    eps, pi = dtype(EPS32), dtype(np.pi)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    a, b, rho = x + eps, z + eps, np.sqrt(x * x + y * y)
    s1, s2 = a * a + y * y, rho * rho + b * b
    dphi, dth = -G[:, 0] / pi, dtype(2) * G[:, 1] / pi
    drho = dth * b / s2
    safe = np.where(rho > 0, rho, dtype(1))
    rx, ry = np.where(rho > 0, x / safe, dtype(0)), np.where(rho > 0, y / safe, dtype(0))
    return np.stack([dphi * (-y / s1) + drho * rx, dphi * (a / s1) + drho * ry, dth * (-rho / s2)], 1)


def pano_pixels(xyz, H, W):
    """(row, col, frow, fcol): make_pano's pixel of every point, trunc(((g + 1) / 2) (res - 1)) in float64, and the fractional position
    inside it (what decides whether fp32 can land in a neighbour)"""
    g = cloud2idx(xyz)
    cx, cy = (g[:, 0] + 1.0) / 2.0 * (W - 1), (g[:, 1] + 1.0) / 2.0 * (H - 1)
    col, row = np.clip(np.trunc(cx), 0, W - 1).astype(np.int64), np.clip(np.trunc(cy), 0, H - 1).astype(np.int64)
    return row, col, cy - row, cx - col


def pano_points(H, W, r, c, fr, fc, d):
    """float32 camera-frame points at depth d that sit at fraction (fr, fc) of pixel (r, c) of an H x W panorama: the inverse of the
    projection, with its two 1e-6 taken off again.  r < H - 1 and c < W - 1 (the last row and column hold only the -z axis and the
    seam); a resolution of one row or column has every point in it, whatever the angle."""
    cy, cx = (np.asarray(r) + fr) / max(H - 1, 1), (np.asarray(c) + fc) / max(W - 1, 1)
    theta, a = np.pi * cy, 2.0 * np.pi * (1.0 - cx) - np.pi
    d = np.asarray(d, F64)
    p = np.stack([d * np.cos(a) * np.sin(theta), d * np.sin(a) * np.sin(theta), d * np.cos(theta)], 1) - np.array([1e-6, 0.0, 1e-6])
    return p.astype(F32)


N_SPECIAL = 9


def special_points(H, W, depths):
    """the nine points every case carries: +z and -z axis (rows 0 and H - 1), the two seam points (columns W - 1 and 0), the origin, and
    four points whose centre pixel lies in row 0 / H - 2 and column 0 / W - 2, so that clamped splat offsets fold onto their own or a
    neighbour's pixel.  depths: six levels for the axis and corner points."""
    r1, c1 = max(H - 2, 0), max(W - 2, 0)
    corner = pano_points(H, W, [0, 0, r1, r1], [0, c1, 0, c1], 0.5, 0.5, depths[2:6])
    axis = np.array([[0, 0, depths[0]], [0, 0, -depths[1]], [-1, -0.0, 0], [-1, 0.0, 0], [0, 0, 0]], F32)
    return np.concatenate([axis, corner])


def pano_case(H, W, n, seed, dup=0, specials=True):
    """A seeded cloud of n points for an H x W panorama: generated points that cover the centre pixels round-robin (several per pixel once
    n exceeds them), each on a depth level of its own; `dup` bit-identical copies of generated points (their own colours: the tie rules
    decide); the special points; all rows shuffled.  -> dict(xyz, rgb (unique rows in (0, 1]), generated (mask), H, W)"""
    rng = np.random.default_rng(seed)
    ns = N_SPECIAL if specials else 0
    ng = n - ns - dup
    assert ng >= 1 and dup <= ng
    hm, wm = max(H - 1, 1), max(W - 1, 1)
    cell = rng.permutation(ng) % (hm * wm)
    level = DEPTH_RATIO ** (1.0 + rng.permutation(ng + 6))
    xyz = pano_points(H, W, cell // wm, cell % wm, rng.uniform(0.25, 0.75, ng), rng.uniform(0.25, 0.75, ng), level[:ng])
    gen = np.ones(ng, bool)
    if dup:
        xyz = np.concatenate([xyz, xyz[rng.choice(ng, dup, replace=False)]])
        gen = np.concatenate([gen, np.ones(dup, bool)])
    if specials:
        xyz = np.concatenate([xyz, special_points(H, W, level[ng:])])
        gen = np.concatenate([gen, np.zeros(ns, bool)])
    perm = rng.permutation(n)
    rgb = rng.uniform(0.01, 1.0, (n, 3)).astype(F32)
    assert len(np.unique(rgb * F32(255), axis=0)) == n
    return dict(xyz=np.ascontiguousarray(xyz[perm]), rgb=rgb, generated=gen[perm], H=H, W=W)


def pass_pairs_case(H, W, seed):
    """One pair of points for every two passes a < b, alone in a 6 x 6 block of pixels: point A sits at P - offset(a), point B at
    P - offset(b), so that pixel P receives pass a from A, pass b from B and nothing else.  B must win whatever the depths (A is the nearer
    one): exchanging any two passes, or ranking depth over the pass, shows at P.  Plus the special points.  -> as pano_case"""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for b in range(9) for a in range(b)]
    per_row = (W - 2) // 6
    assert len(pairs) <= per_row * ((H - 2) // 6)
    r, c = [], []
    for k, (a, b) in enumerate(pairs):
        pr, pc = 1 + 6 * (k // per_row) + 2, 1 + 6 * (k % per_row) + 2
        r += [pr - PANO_PASSES[a][0], pr - PANO_PASSES[b][0]]
        c += [pc - PANO_PASSES[a][1], pc - PANO_PASSES[b][1]]
    ng = len(r)
    level = DEPTH_RATIO ** (1.0 + np.arange(ng + 6))
    xyz = pano_points(H, W, np.array(r), np.array(c), rng.uniform(0.25, 0.75, ng), rng.uniform(0.25, 0.75, ng), level[:ng])
    xyz = np.concatenate([xyz, special_points(H, W, level[ng:])])
    n = len(xyz)
    perm = rng.permutation(n)
    rgb = rng.uniform(0.01, 1.0, (n, 3)).astype(F32)
    assert len(np.unique(rgb * F32(255), axis=0)) == n
    return dict(xyz=np.ascontiguousarray(xyz[perm]), rgb=rgb, generated=np.arange(n)[perm] < ng, H=H, W=W)


def depth_separation(xyz):
    """Condition 2: two points are either equal in |x|, |y|, |z| bit for bit (their squares, and so every evaluation of the norm, agree) or
    their float64 norms differ by a relative gap; -> the smallest such gap (inf when there is one depth only).  Asserted >= DEPTH_GAP:
    a contracted fp32 x*x + y*y + z*z is within 2^-22 of the float64 norm and cannot reorder them."""
    a = np.unique(np.abs(np.asarray(xyz, F32)), axis=0).astype(F64)
    d = np.sort(np.sqrt((a * a).sum(1)))
    if len(d) < 2:
        return np.inf
    return float(((d[1:] - d[:-1]) / d[1:]).min())


# ================================================================================================ make_pano, scatter_min_depth
def make_pano_winners(xyz, H, W, row, col, passes=None, wrap_col0=False, tie_smallest=False):
    """(winner (H W,) int64, -1 where nothing lands; pass (H W,)): per pixel the latest pass, then the smallest depth, then the LARGEST
    index; splat offsets clamped into the image.  Planted: other `passes`, wrap-around instead of the clamp at column 0, the smallest index
    in a tie."""
    passes = PANO_PASSES if passes is None else passes
    p = np.asarray(xyz, F64)
    d, idx = np.sqrt((p * p).sum(1)), np.arange(len(p))
    order = np.lexsort((idx if tie_smallest else -idx, d))            # nearest first, then the tie rule
    winner, wpass = np.full(H * W, -1, np.int64), np.full(H * W, -1, np.int64)
    for k, (dr, dc) in enumerate(passes):
        r, c = np.clip(row + dr, 0, H - 1), col + dc
        if wrap_col0:
            c = np.where(c < 0, W - 1, c)
        pix = (r * W + np.clip(c, 0, W - 1))[order]
        u, first = np.unique(pix, return_index=True)
        winner[u], wpass[u] = order[first], k
    return winner, wpass


def pano_image(winner, rgb, H, W):
    """float32(rgb[winner]) * 255, 0 where nothing landed"""
    img = np.zeros((H * W, 3), F32)
    hit = winner >= 0
    img[hit] = np.asarray(rgb, F32)[winner[hit]] * F32(255)
    return img.reshape(H, W, 3)


def winners_from_image(img, rgb):
    """the point behind every pixel of a make_pano image (colours are unique and non-zero: pano_case), -1 for black"""
    table = {v.tobytes(): i for i, v in enumerate(np.asarray(rgb, F32) * F32(255))}
    flat = np.ascontiguousarray(img, F32).reshape(-1, 3)
    return np.array([-1 if not v.any() else table.get(v.tobytes(), -2) for v in flat], np.int64)


def scatter_min(xyz, H, W, row, col):
    """(zmin float64, arg): per pixel the smallest depth, then the smallest index; empty pixels 0 and n"""
    p = np.asarray(xyz, F64)
    n = len(p)
    d = np.sqrt((p * p).sum(1))
    order = np.lexsort((np.arange(n), d))
    u, first = np.unique((row * W + col)[order], return_index=True)
    zmin, arg = np.zeros(H * W), np.full(H * W, n, np.int64)
    zmin[u], arg[u] = d[order[first]], order[first]
    return zmin, arg


# ================================================================================================ sample_from_img
def sample_taps(coord, H, W, dtype=F64):
    """The footprint of every coordinate: clip to +-0.99 IN FP32 (torch.clip on the fp32 tensor), then ix = ((g + 1) size - 1) / 2 and the
    four taps nw, ne, sw, se with their weights in `dtype`; align_corners=False, zero padding.
    -> dict(inr (n, 2) the clip passes the gradient, ix, iy, wx0, wx1, wy0, wy1, w (n, 4), xx, yy (n, 4), inb (n, 4) tap inside the image)"""
    c = np.asarray(coord, F32).reshape(-1, 2)
    inr = (c >= -LIM32) & (c <= LIM32)
    g = np.clip(c, -LIM32, LIM32).astype(dtype)
    one, two = dtype(1), dtype(2)
    ix, iy = ((g[:, 0] + one) * dtype(W) - one) / two, ((g[:, 1] + one) * dtype(H) - one) / two
    fx0, fy0 = np.floor(ix), np.floor(iy)
    wx1, wx0, wy1, wy0 = ix - fx0, (fx0 + one) - ix, iy - fy0, (fy0 + one) - iy
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], 1)
    xx = fx0.astype(np.int64)[:, None] + np.array([0, 1, 0, 1])
    yy = fy0.astype(np.int64)[:, None] + np.array([0, 0, 1, 1])
    inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    return dict(inr=inr, ix=ix, iy=iy, wx0=wx0, wx1=wx1, wy0=wy0, wy1=wy1, w=w, xx=xx, yy=yy, inb=inb)


def _tap_values(img, t, dtype):
    H, W = img.shape[:2]
    v = np.asarray(img, dtype)[np.clip(t["yy"], 0, H - 1), np.clip(t["xx"], 0, W - 1)]          # (n, 4, 3)
    return np.where(t["inb"][:, :, None], v, dtype(0))


def sample_from_img(img, coord, dtype=F64):
    """(n, 3): the four taps times their weights, summed nw, ne, sw, se"""
    H, W = img.shape[:2]
    t = sample_taps(coord, H, W, dtype)
    v, w = _tap_values(img, t, dtype), t["w"]
    return v[:, 0] * w[:, 0:1] + v[:, 1] * w[:, 1:2] + v[:, 2] * w[:, 2:3] + v[:, 3] * w[:, 3:4]


def sample_from_img_backward(img, coord, gout, dtype=F64, pass_clip=False, keep_border=False):
    """-> dict(grad_coord (n, 2); grad_img (H, W, 3); asum (H, W, 3) the sum of |contribution| per texel channel; gsum (H, W, 3) the sum of
    |gout| over the contributing points; count (H, W) the number of non-zero-weight contributions per texel; bound (H, W, 3): see
    atomic_sum_bound).  grad_coord = [clip passes] (size / 2) <gout, d out / d (ix, iy)>; grad_img[tap] +=
    weight gout for the taps inside the image.  Planted: the clip gradient passed outside +-0.99; a border tap not dropped (it lands in
    the flat buffer's neighbouring texel, as an unchecked address would)."""
    H, W = img.shape[:2]
    t = sample_taps(coord, H, W, dtype)
    v, g = _tap_values(img, t, dtype), np.asarray(gout, dtype).reshape(-1, 3)
    dx = (v[:, 1] - v[:, 0]) * t["wy0"][:, None] + (v[:, 3] - v[:, 2]) * t["wy1"][:, None]
    dy = (v[:, 2] - v[:, 0]) * t["wx0"][:, None] + (v[:, 3] - v[:, 1]) * t["wx1"][:, None]
    sx = g[:, 0] * dx[:, 0] + g[:, 1] * dx[:, 1] + g[:, 2] * dx[:, 2]
    sy = g[:, 0] * dy[:, 0] + g[:, 1] * dy[:, 1] + g[:, 2] * dy[:, 2]
    gc = np.stack([sx * (dtype(W) / dtype(2)), sy * (dtype(H) / dtype(2))], 1)
    if not pass_clip:
        gc = np.where(t["inr"], gc, dtype(0))
    flat = np.clip(t["yy"] * W + t["xx"], 0, H * W - 1)
    keep = np.ones_like(t["inb"]) if keep_border else t["inb"]
    contrib = t["w"][:, :, None] * g[:, None, :]                                                  # (n, 4, 3)
    gi, asum, gsum = np.zeros((H * W, 3), dtype), np.zeros((H * W, 3), dtype), np.zeros((H * W, 3), dtype)
    count = np.zeros(H * W, np.int64)
    live = keep & (t["w"] != 0)
    np.add.at(gi, flat[keep], contrib[keep])
    np.add.at(asum, flat[keep], np.abs(contrib[keep]))
    np.add.at(gsum, flat[live], np.broadcast_to(np.abs(g)[:, None, :], contrib.shape)[live])
    np.add.at(count, flat[live], 1)
    out = dict(grad_coord=gc, grad_img=gi.reshape(H, W, 3), asum=asum.reshape(H, W, 3), gsum=gsum.reshape(H, W, 3), count=count.reshape(H, W))
    out["bound"] = atomic_sum_bound(out, H, W)
    return out


def atomic_sum_bound(m, H, W):
    """What fp32 atomics in ANY order may differ from the float64 grad_img by, per texel channel:
      (count + 3) 2^-24 asum      the fp32 summation bound: count - 1 additions, and the three roundings of a contribution (two weight factors'
                                  product, times gout), each relative to the |contribution|s that asum adds up;
    + 2.5 (W + H) 2^-24 gsum      the weights themselves: ix = ((g + 1) W - 1) / 2 carries the roundings of g + 1 (2^-24), of the product
                                  (2 W 2^-24) and of the - 1 (2 W 2^-24), halved: |d ix| <= 2.5 W 2^-24, likewise iy with H; ix - floor(ix) is
                                  exact, so a weight product is off by at most 2.5 (W + H) 2^-24, times |gout| per contribution.
    Zero where nothing contributes: such a texel must stay exactly 0."""
    u = 2.0 ** -24
    return (m["count"][:, :, None] + 3) * u * m["asum"].astype(F64) + 2.5 * (W + H) * u * m["gsum"].astype(F64)


# ================================================================================================ packers
PANO_FMTS = ("f32", "u8", "f16", "u8p", "u8v")


def levels_image(levels):
    """the float32 image of integer levels: k / 255 by IEEE fp32 division (uint8 -> .float() / 255.)"""
    return (np.asarray(levels).astype(F32) / F32(255)).astype(F32)


def pack_pano(levels, fmt, swap_parity=False, shift_lower=False):
    """The bytes of a packed panorama of integer levels (H, W, 3) in texel layout `fmt`, over the whole padded size: (H + 2) x (W + 2) texels
    with a zero border and alpha 0.
      f32: float4 (r, g, b, 0) of k / 255;  u8: one 32-bit word r | g << 8 | b << 16;  f16: half4 (r, g, b, 0) holding the LEVELS;
      u8p: the u8 word of bordered (yp, xp) at word index ((yp >> 1) (W + 2) + xp) 2 + (yp & 1), (H + 3) >> 1 row pairs (an odd H + 2
           leaves a last half pair: zeros);  u8v: element (yp, xp) = the u8 words of (yp, xp) and (yp + 1, xp), the last row's lower one 0.
    Planted: u8p parity swapped; the u8v lower texel taken from its own row instead of the one below."""
    lv = np.asarray(levels).astype(np.uint32)
    H, W = lv.shape[:2]
    Hp, Wp = H + 2, W + 2
    word = np.zeros((Hp, Wp), np.uint32)
    word[1:H + 1, 1:W + 1] = lv[:, :, 0] | (lv[:, :, 1] << 8) | (lv[:, :, 2] << 16)
    if fmt == "f32":
        out = np.zeros((Hp, Wp, 4), F32)
        out[1:H + 1, 1:W + 1, :3] = levels_image(levels)
    elif fmt == "u8":
        out = word
    elif fmt == "f16":
        out = np.zeros((Hp, Wp, 4), np.float16)
        out[1:H + 1, 1:W + 1, :3] = lv.astype(np.float16)
    elif fmt == "u8p":
        out = np.zeros(((H + 3) >> 1) * Wp * 2, np.uint32)
        yp, xp = np.mgrid[0:Hp, 0:Wp]
        par = (yp & 1) ^ 1 if swap_parity else yp & 1
        out[((yp >> 1) * Wp + xp) * 2 + par] = word
    elif fmt == "u8v":
        out = np.zeros((Hp, Wp, 2), np.uint32)
        out[:, :, 0] = word
        if shift_lower:
            out[:, :, 1] = word
        else:
            out[:-1, :, 1] = word[1:]
    else:
        raise ValueError(fmt)
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1)


def pano_bytes(H, W, fmt):
    return {"f32": 16, "u8": 4, "f16": 8, "u8v": 8}[fmt] * (H + 2) * (W + 2) if fmt != "u8p" else ((H + 3) >> 1) * (W + 2) * 8


def cloud_stride(n):
    return (n + 255) // 256 * 256


def pack_cloud_sets(xyz, rgbs, order=None, per_launch=16, second_launch_at_0=False):
    """(3 + 3 k, stride) float32: planes x, y, z, then (-r, -g, -b) per colour set, each in packed order (slot s holds point order[s]) and
    padded with +0.0 to a multiple of 256.  One colour set is pcl_cloud_pack's six planes.  Planted: a launch after the first (`per_launch`
    sets each) writes its colour planes from set 0 on, over the first launch's, and leaves its own unwritten."""
    xyz = np.asarray(xyz, F32)
    n = len(xyz)
    o = np.arange(n) if order is None else np.asarray(order)
    out = np.zeros((3 + 3 * len(rgbs), cloud_stride(n)), F32)
    out[:3, :n] = xyz[o].T
    for k, rgb in enumerate(rgbs):
        at = k % per_launch if second_launch_at_0 else k
        out[3 + 3 * at:6 + 3 * at, :n] = -np.asarray(rgb, F32)[o].T
    return out


def pack_weights(w, order=None):
    w = np.asarray(w, F32)
    out = np.zeros(cloud_stride(len(w)), F32)
    out[:len(w)] = w if order is None else w[np.asarray(order)]
    return out


def bits(a):
    """float32 array -> its words: comparisons that tell -0.0 from +0.0"""
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ================================================================================================ Morton order
MORTON_TOP = 2097151                    # 2^21 - 1


def lattice(k):
    """float32 coordinates k 2^-10 of integer k in [0, 2^21 - 1]: with both extremes on an axis its scale (2^21 - 1) / (hi - lo) is exactly
    2^10 and every quantised coordinate is exactly k"""
    k = np.asarray(k)
    assert k.min() >= 0 and k.max() <= MORTON_TOP
    return (k.astype(F64) / 1024.0).astype(F32)


def _spread21(v):
    out = np.zeros_like(v)
    for b in range(21):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_keys(xyz, box_rows=None):
    """63-bit keys: per axis trunc(clamp((x - lo) (2^21 - 1) / (hi - lo), 0, 2^21 - 1)) in fp32 (scale 0 when hi == lo), x bits at 3 b,
    y at 3 b + 1, z at 3 b + 2.  Planted: a bounding box of the first `box_rows` points only."""
    p = np.asarray(xyz, F32)
    src = p if box_rows is None else p[:box_rows]
    lo, hi = src.min(0), src.max(0)
    top = F32(MORTON_TOP)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(hi > lo, top / (hi - lo), F32(0)).astype(F32)
    q = np.clip((p - lo) * sc, F32(0), top).astype(np.uint64)
    return _spread21(q[:, 0]) | (_spread21(q[:, 1]) << np.uint64(1)) | (_spread21(q[:, 2]) << np.uint64(2))


def morton_order(xyz, box_rows=None):
    """the stable argsort of the keys: equal keys keep their input order"""
    return np.argsort(morton_keys(xyz, box_rows), kind="stable")
