"""The voxel grid's rules as a numpy model, written from their text (include/piccolo_hip.h) — what the device results
are compared with BIT FOR BIT — and a loop-per-point model of the same text that the numpy one is checked against.

    cell      per axis floor((double)x / (double)voxel), origin 0, inside [-2^20, 2^20)
    ids       voxels numbered in first-occurrence order: first[v] (the voxel's lowest point index) increases strictly with v
    centroid  q = llrint((double)a * 65536) (half to even), S[v] = sum q as exact int64, (float)((double)S / ((double)count * 65536.0))
    weight    1 where count[cell_i] <= cap, else (float)((double)cap / (double)count[cell_i])
    first     the representative of a voxel is its lowest-index point, copied bit for bit
"""
import numpy as np

HALF = 1 << 20
BAD_NONFINITE, BAD_CELL, BAD_MAGNITUDE = 1, 2, 4


def cells(xyz, voxel):
    """(N, 3) int64 cells of float32 points"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.floor(x / np.float64(voxel)).astype(np.int64)


def bad_bits(values, voxel=None):
    """the bad set of an array of float32 values (coordinates with `voxel`, colours without)"""
    a = np.asarray(values, np.float32)
    bits = 0
    finite = np.isfinite(a)
    if not finite.all():
        bits |= BAD_NONFINITE
    if (np.abs(a[finite]) >= 32768).any():
        bits |= BAD_MAGNITUDE
    if voxel is not None:
        c = np.floor(a[finite].astype(np.float64) / np.float64(voxel))
        if ((c < -HALF) | (c >= HALF)).any():
            bits |= BAD_CELL
    return bits


def grid(xyz, voxel):
    """-> (cell_of_point (N,) int32, count (V,) int32, first (V,) int64)"""
    c = cells(xyz, voxel) + HALF
    assert c.min() >= 0 and c.max() < 2 * HALF
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first, inverse, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")                # unique's sorted-key order -> first-occurrence order
    rank = np.empty_like(by_first)
    rank[by_first] = np.arange(len(by_first))
    return rank[inverse.reshape(-1)].astype(np.int32), count[by_first].astype(np.int32), first[by_first].astype(np.int64)


def quantise(a):
    return np.rint(np.asarray(a, np.float32).astype(np.float64) * 65536.0).astype(np.int64)


def centroids(values, cell, count):
    """(V, 3) float32 centroids of (N, 3) float32 values"""
    q = quantise(values)
    S = np.zeros((len(count), 3), np.int64)
    np.add.at(S, np.asarray(cell, np.int64), q)
    return (S.astype(np.float64) / (count.astype(np.float64) * 65536.0)[:, None]).astype(np.float32)


def weights(cell, count, cap=1):
    cnt = count[np.asarray(cell, np.int64)].astype(np.float64)
    return np.where(cnt <= cap, np.float32(1.0), (np.float64(cap) / cnt).astype(np.float32)).astype(np.float32)


def downsample(xyz, rgb, voxel, how="centroid"):
    """-> (xyz', rgb', count, first), what utils.voxel_downsample returns"""
    xyz, rgb = np.asarray(xyz, np.float32), np.asarray(rgb, np.float32)
    cell, count, first = grid(xyz, voxel)
    if how == "first":
        return xyz[first], rgb[first], count, first
    return centroids(xyz, cell, count), centroids(rgb, cell, count), count, first


# ------------------------------------------------------------------------------------------------ one point at a time
def brute(xyz, rgb, voxel, cap=1):
    """The same text with a Python loop per point and exact Python integers: (cell, count, first, xyz', rgb', w)"""
    import math
    xyz, rgb = np.asarray(xyz, np.float32), np.asarray(rgb, np.float32)
    ids, cell, count, first, sums = {}, [], [], [], []
    for i in range(len(xyz)):
        key = tuple(int(math.floor(float(xyz[i, k]) / float(voxel))) for k in range(3))
        assert all(-HALF <= c < HALF for c in key)
        if key not in ids:
            ids[key] = len(ids)
            count.append(0)
            first.append(i)
            sums.append([0] * 6)
        v = ids[key]
        cell.append(v)
        count[v] += 1
        for k in range(6):
            a = float(xyz[i, k]) if k < 3 else float(rgb[i, k - 3])
            sums[v][k] += int(round(a * 65536.0))          # (Python's round: half to even; a * 65536 is exact in a double)
    cen = np.array([[np.float32(float(s) / (float(c) * 65536.0)) for s in row] for row, c in zip(sums, count)], np.float32).reshape(-1, 6)
    w = np.array([np.float32(1.0) if count[v] <= cap else np.float32(float(cap) / float(count[v])) for v in cell], np.float32)
    return (np.array(cell, np.int32), np.array(count, np.int32), np.array(first, np.int64), cen[:, :3].copy(), cen[:, 3:].copy(), w)
