"""The numpy model of the alignment recipe (include/piccolo_hip.h) and the scenes its tests share.

Moments are integers; the scatter matrix A = count S2 - S1 S1^T is computed in Python integers (exact) and rounded once to double;
numpy.linalg.eigh supplies the eigen part.  The vote is restated operation by operation: every elementwise step is one IEEE double
operation in the device's order (numpy fuses nothing), every accumulation an integer sum — fed the device's own normals and planarities it
must return the device's record bit for bit.  The one transcendental, the arctangent that names a wall normal's azimuth bin, decides only
which bin a voxel falls into.
"""
import math

import numpy as np

GRID, ROUNDS, YAW_BINS = 64, 3, 360
COS_CONE = 0.99619469809174555            # cos 5 degrees
SIN_WALL = 0.17364817766693033            # sin 10 degrees
YAW_HALF = 3.0
Q = 1048576.0
DEG = 57.295779513082323

# The scenes of the end-to-end tests: (maker, tilt degrees, azimuth of the tilt axis degrees, yaw degrees), 20,000 points, 10 cm voxels
SCENES = (("box", 0.0, 0.0, 0.0), ("box", 7.0, 30.0, 20.0), ("furnished", 7.0, 200.0, -40.0), ("scanned", 25.0, 30.0, 20.0),
          ("furnished", 25.0, 200.0, 0.0), ("scanned", 0.0, 0.0, -40.0))
SCENE_POINTS, SCENE_VOXEL, SCENE_MIN_COUNT, NOISE = 20_000, 0.1, 3, 0.002
# THE MODEL'S OWN ERRORS on these scenes, in SCENES' order, as measured on the CPU (tests/test_align_model.py prints and re-checks them):
# the angle between the model's up and the planted up, and the yaw error modulo 90 degrees, in degrees.  Nothing derives them — the bin and
# cone widths make the error scene-dependent; the GPU tests assert TWICE these.
MODEL_UP_ERROR_DEG = (0.2720, 0.3994, 0.1914, 0.1288, 0.3360, 0.0209)
MODEL_YAW_ERROR_DEG = (0.3961, 0.5042, 1.0425, 0.3178, 0.8027, 0.2516)
# For the CPU re-check alone: how far a re-measurement may lie from the recorded figures (they are rounded to 1e-4 degrees, and another
# LAPACK's eigh may move a voxel across a cone's edge, which shifts a weighted mean over a thousand voxels by a few thousandths of a degree)
MODEL_RECHECK_DEG = 0.01
# the noisy box room of the normals test, and the share of its eligible voxels the eigen-gap condition may leave out
NORMALS_SCENE = dict(points=20_000, voxel=0.25, min_count=8)
GAP, GAP_SHARE = 1e-3, 0.10


# ------------------------------------------------------------------------------------------------ scenes
def _face_normals(xyz, furnished):
    """the axis of the face every point of a synth room lies on, as unit vectors (N, 3)"""
    from piccolo_amd import synth
    planes = [(axis, sign * synth.ROOM[axis] / 2) for axis in range(3) for sign in (-1.0, 1.0)]
    if furnished:
        planes += [(axis, c[axis] + sign * sz[axis] / 2) for c, sz in synth._FURNITURE for axis in range(3) for sign in (-1.0, 1.0)]
    out = np.zeros((len(xyz), 3))
    done = np.zeros(len(xyz), bool)
    for axis, coord in planes:
        m = ~done & (np.abs(xyz[:, axis].astype(np.float64) - coord) < 1e-5)
        out[m, axis] = 1.0
        done |= m
    assert done.all()
    return out


def plant_rotation(tilt_deg, azimuth_deg, yaw_deg):
    """the room turned by yaw about z, then tilted by `tilt` about the horizontal axis at `azimuth`: x_cloud = R x_room"""
    t, a, y = (math.radians(v) for v in (tilt_deg, azimuth_deg, yaw_deg))
    k = np.array([math.cos(a), math.sin(a), 0.0])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    tilt = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    return tilt @ rz


def planted_scene(kind, tilt_deg, azimuth_deg, yaw_deg, n=SCENE_POINTS, seed=5):
    """(xyz float32 (N, 3), rgb, planted up (3,), planted yaw degrees): a synth room with NOISE metres of Gaussian noise along its faces'
    normals (voxels are not exactly singular), turned by plant_rotation"""
    from piccolo_amd import synth
    xyz, rgb = {"box": synth.box_room, "furnished": synth.furnished_room, "scanned": synth.scanned_room}[kind](n, seed)
    rng = np.random.default_rng(1000 + seed)
    noisy = xyz.astype(np.float64) + _face_normals(xyz, kind == "furnished") * rng.normal(0.0, NOISE, size=(len(xyz), 1))
    R = plant_rotation(tilt_deg, azimuth_deg, yaw_deg)
    return (noisy @ R.T).astype(np.float32), rgb, R[:, 2].copy(), yaw_deg


def exact_plane(n, z=0.25, seed=3):
    """n points of the plane z = const on a 1 / 1024 lattice: every coordinate, and every llrint(a 65536), is exact"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 1024, size=(n, 2)) / 1024.0
    return np.concatenate([xy, np.full((n, 1), z)], axis=1).astype(np.float32)


def up_error_deg(up, planted):
    """the unsigned angle between two directions, in degrees (by the arctangent: an arccosine near 1 has a floor of 1e-8 radians' root)"""
    up, planted = np.asarray(up, np.float64), np.asarray(planted, np.float64)
    return math.degrees(math.atan2(float(np.linalg.norm(np.cross(up, planted))), abs(float(np.dot(up, planted)))))


def yaw_error_deg(yaw_rad, planted_deg):
    d = math.degrees(yaw_rad) - planted_deg
    return abs(d - 90.0 * round(d / 90.0))


# ------------------------------------------------------------------------------------------------ grid, moments, normals
def quantise(a):
    return np.rint(np.asarray(a, np.float32).astype(np.float64) * 65536.0).astype(np.int64)


def grid_model(xyz, voxel):
    """(cell (N,), count (V,), first (V,)) of pcl_voxel_grid: voxels numbered in first-occurrence order"""
    cells = np.floor(np.asarray(xyz, np.float32).astype(np.float64) / float(voxel)).astype(np.int64)
    _, first, inverse = np.unique(cells, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    cell = rank[inverse.reshape(-1)]
    return cell.astype(np.int32), np.bincount(cell).astype(np.int32), first[order].astype(np.int64)


def moments_model(xyz, cell, first, nvoxels, skip=None):
    """(V, 9) int64: S1 (3) and S2 (xx xy xz yy yz zz) of d = q(x_i) - q(x_first[v]); skip: a bool mask of points that add nothing"""
    q = quantise(xyz)
    cell = np.asarray(cell, np.int64)
    d = q - q[np.asarray(first, np.int64)[cell]]
    rows = np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                     d[:, 2] * d[:, 2]], axis=1)
    if skip is not None:
        rows = rows[~skip]
        cell = cell[~skip]
    out = np.zeros((int(nvoxels), 9), np.int64)
    np.add.at(out, cell, rows)
    return out


def covariance_model(moments, count):
    """(V, 3, 3) float64: A = count S2 - S1 S1^T in Python integers, each entry rounded once to double, / (count count 2^32)"""
    V = len(count)
    out = np.zeros((V, 3, 3))
    pairs = ((0, 0, 3), (0, 1, 4), (0, 2, 5), (1, 1, 6), (1, 2, 7), (2, 2, 8))
    for v in range(V):
        c = int(count[v])
        m = [int(x) for x in moments[v]]
        den = float(c) * float(c) * 4294967296.0
        for p, q, k in pairs:
            out[v, p, q] = out[v, q, p] = float(c * m[k] - m[p] * m[q]) / den
    return out


def normals_model(moments, count):
    """(eigenvalues (V, 3) ascending, the unit eigenvector of the smallest (V, 3)) by numpy.linalg.eigh on covariance_model's matrices"""
    w, v = np.linalg.eigh(covariance_model(moments, count))
    return w, v[:, :, 0]


# ------------------------------------------------------------------------------------------------ the vote
def _voters(normal, planarity, count, fold):
    p = np.asarray(planarity, np.float32)
    cnt = np.asarray(count, np.int64)
    ok = (cnt > 0) & (p > 0) & (p <= 1)
    w = cnt * np.rint(np.where(ok, p, 0).astype(np.float64) * 4096.0).astype(np.int64)
    n = np.asarray(normal, np.float32).astype(np.float64)
    nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
    with np.errstate(invalid="ignore"):
        ok &= (w > 0) & (nn > 0.25) & (nn < 4.0)
    n = n[ok]
    if fold:
        n = np.where((n[:, 2] < 0.0)[:, None], -n, n)
    return w[ok], n


def _unit(x, y, z):
    length = math.sqrt(x * x + y * y + z * z)
    return np.array([x / length, y / length, z / length])


def up_rotation(a):
    k = 1.0 / (1.0 + a[2])
    r01 = -((a[0] * a[1]) * k)
    return np.array([[1.0 - (a[0] * a[0]) * k, r01, -a[0]], [r01, 1.0 - (a[1] * a[1]) * k, -a[1]],
                     [a[0], a[1], 1.0 - (a[0] * a[0] + a[1] * a[1]) * k]])


def _half_angle(c, s):
    if c >= 0.0:
        ch = math.sqrt((1.0 + c) / 2.0)
        return ch, s / (2.0 * ch)
    sh = math.sqrt((1.0 - c) / 2.0)
    if s < 0.0:
        sh = -sh
    return s / (2.0 * sh), sh


def _isum(w, x):
    """sum of w * llrint(x 2^20), exact"""
    return int(np.sum(w * np.rint(x * Q).astype(np.int64)))


def vote_model(normal, planarity, count, max_tilt=40.0, yaw=False):
    """ops.align_vote's dict from (V, 3) float32 normals, (V,) float32 planarities and (V,) counts"""
    T = math.tan(float(max_tilt) * 0.017453292519943295)
    out = {"up": np.array([0.0, 0.0, 1.0]), "rot": np.eye(3), "cos_tilt": 1.0, "sin_tilt": 0.0, "cos_yaw": 1.0, "sin_yaw": 0.0, "status": 0}
    weights = [0, 0, 0, 0]
    w, n = _voters(normal, planarity, count, True)
    up = n[:, 2] > 0.0
    wu, nu = w[up], n[up]
    gu, gv = nu[:, 0] / nu[:, 2], nu[:, 1] / nu[:, 2]
    keep = gu * gu + gv * gv <= T * T
    wu, gu, gv = wu[keep], gu[keep], gv[keep]
    scale = float(GRID // 2) / T
    bx = np.clip(np.floor((gu + T) * scale).astype(np.int64), 0, GRID - 1)
    by = np.clip(np.floor((gv + T) * scale).astype(np.int64), 0, GRID - 1)
    hist = np.zeros(GRID * GRID, np.int64)
    np.add.at(hist, by * GRID + bx, wu)
    weights[0] = int(hist.sum())
    best = int(np.argmax(hist))
    out["hist"] = hist
    if hist[best] <= 0:
        out["status"] = 1
    else:
        step = T / float(GRID // 2)
        cu, cv = (float(best % GRID) + 0.5) * step - T, (float(best // GRID) + 0.5) * step - T
        e = _unit(cu, cv, 1.0)
        for _ in range(ROUNDS):
            m = n[:, 0] * e[0] + n[:, 1] * e[1] + n[:, 2] * e[2] >= COS_CONE
            sums = [_isum(w[m], n[m, c]) for c in range(3)]
            weights[1] = int(w[m].sum())
            e = _unit(float(sums[0]), float(sums[1]), float(sums[2]))
        r = up_rotation(e)
        out["up"], out["cos_tilt"], out["sin_tilt"] = e, float(e[2]), math.sqrt(e[0] * e[0] + e[1] * e[1])
        if yaw:
            w2, n2 = _voters(normal, planarity, count, False)
            x = (r[0, 0] * n2[:, 0] + r[0, 1] * n2[:, 1]) + r[0, 2] * n2[:, 2]
            y = (r[1, 0] * n2[:, 0] + r[1, 1] * n2[:, 1]) + r[1, 2] * n2[:, 2]
            z = (r[2, 0] * n2[:, 0] + r[2, 1] * n2[:, 1]) + r[2, 2] * n2[:, 2]
            h = np.sqrt(x * x + y * y)
            wall = (np.abs(z) <= SIN_WALL) & (h > 0.0)
            w2, x, y, h = w2[wall], x[wall], y[wall], h[wall]
            c1, s1 = x / h, y / h
            c2, s2 = c1 * c1 - s1 * s1, 2.0 * (c1 * s1)
            c4, s4 = c2 * c2 - s2 * s2, 2.0 * (c2 * s2)
            deg = np.arctan2(y, x) * DEG
            fold = deg - 90.0 * np.floor(deg / 90.0)
            yh = np.zeros(YAW_BINS, np.int64)
            np.add.at(yh, np.clip(np.floor(fold * 4.0).astype(np.int64), 0, YAW_BINS - 1), w2)
            weights[2] = int(yh.sum())
            out["yaw_hist"] = yh
            bi = int(np.argmax(yh))
            C = S = 0
            if yh[bi] > 0:
                diff = fold - (float(bi) + 0.5) * 0.25
                diff = diff - 90.0 * np.rint(diff / 90.0)
                m = np.abs(diff) <= YAW_HALF
                C, S, weights[3] = _isum(w2[m], c4[m]), _isum(w2[m], s4[m]), int(w2[m].sum())
            length = math.sqrt(float(C) * float(C) + float(S) * float(S))
            if weights[3] <= 0 or not length > 0.0:
                out["status"] = 2
            else:
                c2h, s2h = _half_angle(float(C) / length, float(S) / length)
                cy, sy = _half_angle(c2h, s2h)
                out["cos_yaw"], out["sin_yaw"] = cy, sy
                r = np.stack([cy * r[0] + sy * r[1], cy * r[1] - sy * r[0], r[2]])
        out["rot"] = r
    out["tilt"], out["yaw"] = math.atan2(out["sin_tilt"], out["cos_tilt"]), math.atan2(out["sin_yaw"], out["cos_yaw"])
    out["weights"] = tuple(weights)
    return out


def align_model(xyz, voxel, min_count, max_tilt=40.0, yaw=False):
    """the whole recipe on the CPU, eigh in place of the device's Jacobi: (vote_model's dict, normals, planarity, count)"""
    cell, count, first = grid_model(xyz, voxel)
    lam, vec = normals_model(moments_model(xyz, cell, first, len(count)), count)
    ok = (count >= min_count) & (lam[:, 2] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        planarity = np.where(ok, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0).astype(np.float32)
    normal = np.where(ok[:, None], vec, 0.0).astype(np.float32)
    return vote_model(normal, planarity, count, max_tilt, yaw), normal, planarity, count


# ------------------------------------------------------------------------------------------------ transform and pose mapping
def transform_model(xyz, rot, trans):
    """pcl_align_transform_cloud in float32 numpy: d = x - a, out_r = (R_r0 d_0 + R_r1 d_1) + R_r2 d_2"""
    x, r, a = np.asarray(xyz, np.float32), np.asarray(rot, np.float32).reshape(3, 3), np.asarray(trans, np.float32).reshape(3)
    d = x - a[None, :]
    return np.stack([(r[k, 0] * d[:, 0] + r[k, 1] * d[:, 1]) + r[k, 2] * d[:, 2] for k in range(3)], axis=1)


def random_rotation(rng):
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
