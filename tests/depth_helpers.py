"""Reference semantics of the scatter-min depth mask's z-buffers (csrc/pcl_depth.hip) for
tests/test_zpass_exact.py — not a test module.  Plain numpy, float64.

A z-buffer is a min-reduction of integer keys: every z-pass form must leave the same words, and those words are a function of the
occluder samples alone.  The model: sample s = packed point s * stride, p = R (x - t) in float64,
    phi = atan2(py, px + 1e-6)          e = atan2(pz + 1e-6, rho)
    colf = (1/2 - phi / 2 pi)(Wd - 1)   rowf = (1/2 - e / pi)(Hd - 1)        cell = (trunc rowf, trunc colf)
    val = |p|^2 (1 + tau)^2             (the word: the fp32 bit pattern of val; 0x7f800000 = an empty cell)
BAND.  A kernel that works in fp32 may put a sample that lies within a hair of a cell border into the neighbouring cell.  A sample is a
BORDER sample when rowf or colf lies within delta of an integer, otherwise INTERIOR; delta = 3 x the largest difference between the
float32 and the float64 evaluation of rowf / colf over the case's samples (the model's own fp32-vs-fp64 gap; x 3: DESIGN.md section 2),
rho = 3 x the largest relative fp32-vs-fp64 difference of val.  Neither is a chosen number.
RULE, for a z-buffer Z:
  (a) no sample is lost: every interior sample s has Z[cell(s)] <= val(s) (1 + rho);
  (b) nothing is invented: every word that is not 0x7f800000 lies within rho (relative) of val(s) of a CANDIDATE s of its cell — an
      interior sample of the cell, or a border sample whose band reaches it (columns wrap at the seam, rows are clamped).
Together they pin every cell whose candidates are all interior to the true minimum within rho."""
import collections
import types

import numpy as np

Z_INF = 0x7F800000
NQ = 768                    # pcl_zpass_kernel: queue capacity of the second window
BORDER_CAP = 0.01           # a case may leave at most this share of its samples to the band (a cap on what a test leaves out)
LEFT_OUT_CAP = 0.015        # the mark / lookup check: border points plus threshold ties

# name -> (cloud: points used (None: all) and Morton sort, grid (Hd, Wd), occluder stride, tau)
CASES = {
    "W1": dict(npts=None, sort=True, grid=(64, 256), stride=1, tau=0.0),      # window 48 x 128 + second window, 4096 samples per block
    "W2": dict(npts=None, sort=False, grid=(64, 256), stride=1, tau=0.0),     # the same, the queue overflowing
    "W3": dict(npts=None, sort=True, grid=(128, 256), stride=1, tau=0.0),     # window 64 x 128, 2048 per block (not dense)
    "W4": dict(npts=None, sort=True, grid=(64, 128), stride=2, tau=0.0),      # dense window, stride-2 quads, window as wide as the grid
    "W5": dict(npts=None, sort=True, grid=(64, 128), stride=4, tau=0.0),      # not dense, stride-4 quads
    "W6": dict(npts=None, sort=True, grid=(37, 131), stride=3, tau=0.0),      # dense window, generic stride, odd width
    "W7": dict(npts=None, sort=True, grid=(64, 256), stride=1, tau=0.1),      # as W1 with tol2 != 1
    "C1": dict(npts=None, sort=True, grid=(24, 40), stride=1, tau=0.0),       # coarse-tile cache
    "C2": dict(npts=None, sort=True, grid=(37, 100), stride=3, tau=0.0),      # cache, Hd not a multiple of 8, Wd not of 16
    "T1": dict(npts=5, sort=True, grid=(2, 2), stride=4, tau=0.0),            # nz = 2
    "T2": dict(npts=1, sort=True, grid=(16, 32), stride=1, tau=0.0),          # nz = 1
}
B_POSES = 3


def occluder_scene(n=27015):
    """box room + a second, smaller box inside it (test_hip_parity._occluder_scene): 33,768 points = 8 x 4096 + 1000"""
    from piccolo_amd import synth
    xyz, rgb = synth.box_room(n, 17)
    inner, inner_rgb = synth.box_room(n // 4, 18)
    xyz = np.concatenate([xyz, inner * 0.25 + np.array([1.5, 1.0, 0.0], np.float32)]).astype(np.float32)
    rgb = np.concatenate([rgb, inner_rgb]).astype(np.float32)
    return xyz, rgb


def case_poses():
    from piccolo_amd import synth
    t_gt, ypr_gt = synth.gt_pose(17)
    return synth.start_poses(t_gt, ypr_gt, B_POSES, seed=17, sigma_t=0.5, sigma_r=0.5)


def case_points(case, xyz, rgb):
    k = CASES[case]["npts"]
    return (xyz, rgb) if k is None else (xyz[:k], rgb[:k])


# ------------------------------------------------------------------------------------------------- the float64 model
def camera_points(xyz, t, ypr, dtype):
    """R (x - t), every operation in `dtype`"""
    from piccolo_amd import synth
    R = synth.rot_from_ypr_np(ypr).astype(dtype)
    return (xyz.astype(dtype) - np.asarray(t).astype(dtype)[None, :]) @ R.T


def project(cam, Hd, Wd, tau):
    """(rowf, colf, d2, val) of camera-frame points, every operation in cam's dtype"""
    f = cam.dtype.type
    px, py, pz = cam[:, 0], cam[:, 1], cam[:, 2]
    phi = np.arctan2(py, px + f(1e-6))
    e = np.arctan2(pz + f(1e-6), np.sqrt(px * px + py * py))
    colf = (f(0.5) - phi / f(2.0 * np.pi)) * f(Wd - 1)
    rowf = (f(0.5) - e / f(np.pi)) * f(Hd - 1)
    d2 = px * px + py * py + pz * pz
    one_tau = f(1) + f(np.float32(tau))                  # (the entry point takes tau as a float)
    tol2 = one_tau * one_tau
    out = (rowf, colf, d2, d2 * tol2)
    assert all(v.dtype == cam.dtype for v in out)
    return out


# float64 rowf / colf / d2 / val of EVERY packed point of one pose (the occluder samples: every stride-th)
PoseModel = collections.namedtuple("PoseModel", "rowf colf d2 val")


class CaseModel:
    def __init__(self, packed_xyz, trans, rot, grid, stride, tau):
        """packed_xyz: the points in PACKED order (xyz[order]); delta / rho from the samples of all poses of the case"""
        self.Hd, self.Wd = int(grid[0]), int(grid[1])
        self.stride, self.tau, self.n = int(stride), float(tau), len(packed_xyz)
        self.tol2 = (1.0 + float(np.float32(tau))) ** 2
        self.poses, self.gap_cell, self.gap_val = [], 0.0, 0.0
        for b in range(len(trans)):
            r64, c64, d64, v64 = project(camera_points(packed_xyz, trans[b], rot[b], np.float64), self.Hd, self.Wd, tau)
            r32, c32, _, v32 = project(camera_points(packed_xyz, trans[b], rot[b], np.float32), self.Hd, self.Wd, tau)
            s = slice(None, None, self.stride)
            self.gap_cell = max(self.gap_cell, float(np.abs(r32[s] - r64[s]).max()), float(np.abs(c32[s] - c64[s]).max()))
            self.gap_val = max(self.gap_val, float((np.abs(v32[s] - v64[s]) / v64[s]).max()))
            self.poses.append(PoseModel(r64, c64, d64, v64))
        self.delta, self.rho = 3.0 * self.gap_cell, 3.0 * self.gap_val

    # -- per pose, over the points `sel` (a slice; default: the occluder samples)
    def samples(self):
        return slice(None, None, self.stride)

    def border(self, b, sel=None):
        p, sel = self.poses[b], self.samples() if sel is None else sel
        r, c = p.rowf[sel], p.colf[sel]
        return (np.abs(r - np.rint(r)) < self.delta) | (np.abs(c - np.rint(c)) < self.delta)

    def cell(self, b, sel=None):
        """the model's own cell of each point"""
        p, sel = self.poses[b], self.samples() if sel is None else sel
        row = np.clip(np.floor(p.rowf[sel]).astype(np.int64), 0, self.Hd - 1)
        col = np.clip(np.floor(p.colf[sel]).astype(np.int64), 0, self.Wd - 1)
        return row * self.Wd + col

    def candidates(self, b):
        """(cell, sample) pairs without duplicates: every cell a sample may legitimately land in.  Rows: trunc(rowf -+ delta), clamped;
        columns: trunc(colf -+ delta) modulo Wd, and column 0 for a sample within delta of the seam's far side (phi = -pi against +pi)."""
        p, s = self.poses[b], self.samples()
        r, c, d = p.rowf[s], p.colf[s], self.delta
        rows = [np.clip(np.floor(r + e).astype(np.int64), 0, self.Hd - 1) for e in (-d, d)]
        hi = np.floor(c + d).astype(np.int64)
        cols = [np.floor(c - d).astype(np.int64) % self.Wd, hi % self.Wd, np.where(c + d >= self.Wd - 1, 0, hi % self.Wd)]
        nz = len(r)
        key = np.unique(np.concatenate([(rr * self.Wd + cc) * nz + np.arange(nz) for rr in rows for cc in cols]))
        return key // nz, key % nz


def words_to_f64(Z):
    return np.ascontiguousarray(Z, dtype=np.uint32).view(np.float32).astype(np.float64)


def values_to_words(v):
    """float64 values (inf: empty) -> the z-buffer's words"""
    return np.asarray(v, np.float64).astype(np.float32).view(np.uint32)


def check_zbuffer(cm, b, Z):
    """The rule for pose b's z-buffer -> border_share, lost (samples that violate (a)), invented (cells that violate (b)), worst (the largest
    relative error of a word against the true minimum over the cells whose candidates are all interior), pure_cells (how many those are)"""
    Z = np.ascontiguousarray(Z, dtype=np.uint32).reshape(-1)
    assert Z.size == cm.Hd * cm.Wd
    Zf = words_to_f64(Z)
    val = cm.poses[b].val[cm.samples()]
    border, cell = cm.border(b), cm.cell(b)
    out = types.SimpleNamespace()
    out.border_share = float(border.mean())
    interior = np.nonzero(~border)[0]
    with np.errstate(invalid="ignore"):
        ok_a = Zf[cell[interior]] <= val[interior] * (1.0 + cm.rho)                  # (a NaN word fails)
    out.lost = interior[~ok_a]
    ccell, csamp = cm.candidates(b)
    with np.errstate(invalid="ignore"):
        hit = np.abs(Zf[ccell] - val[csamp]) <= cm.rho * val[csamp]
    matched = np.zeros(Z.size, bool)
    matched[ccell[hit]] = True
    out.invented = np.nonzero((Z != Z_INF) & ~matched)[0]                           # (a cell without candidates matches nothing)
    touched = np.zeros(Z.size, bool)
    touched[ccell[border[csamp]]] = True
    true_min = np.full(Z.size, np.inf)
    np.minimum.at(true_min, cell[interior], val[interior])
    pure = np.isfinite(true_min) & ~touched
    out.pure_cells = int(pure.sum())
    with np.errstate(invalid="ignore"):
        err = np.abs(Zf[pure] / true_min[pure] - 1.0)
    out.worst = float(np.nan_to_num(err, nan=np.inf).max()) if out.pure_cells else 0.0
    return out


def reference_zbuffer(cm, b, skip=None):
    """the model's own z-buffer (every sample in its own cell, float64 minimum rounded to fp32); skip: a sample index left out"""
    val, cell = cm.poses[b].val[cm.samples()], cm.cell(b)
    keep = np.ones(len(val), bool)
    if skip is not None:
        keep[skip] = False
    z = np.full(cm.Hd * cm.Wd, np.inf)
    np.minimum.at(z, cell[keep], val[keep])
    return values_to_words(z)


def expected_visible(cm, b, Z):
    """-> (expect, decided), one entry per packed point: visible = d2 <= Z[cell] (the contract of pcl_depth_mask: |p| <= (1 + tau) zmin,
    Z = (zmin (1 + tau))^2) for every point the model can decide — interior, and d2 further than rho (relative) from Z[cell].  Of the
    threshold ties one kind is decidable too, and with tau = 0 it is every cell's own minimum: an occluder sample that is interior and
    whose val lies below every other candidate's of its cell by more than rho wrote Z[cell] itself (rule (a)/(b)), and tol2 = 1 makes
    the word its own d2 — the mark pass recomputes it with the same instructions, so the sample is visible."""
    Zf, p, every = words_to_f64(Z), cm.poses[b], slice(None)
    zc = Zf[cm.cell(b, every)]
    with np.errstate(invalid="ignore"):
        expect = p.d2 <= zc
        decided = ~cm.border(b, every) & (np.isinf(zc) | (np.abs(p.d2 - zc) > cm.rho * zc))
    if cm.tol2 == 1.0:
        val = p.val[cm.samples()]
        ccell, csamp = cm.candidates(b)
        o = np.lexsort((val[csamp], ccell))
        ccell, csamp = ccell[o], csamp[o]
        first = np.r_[True, ccell[1:] != ccell[:-1]]
        second = np.full(len(ccell), np.inf)                                         # the runner-up's val, at each cell's first entry
        nxt = np.r_[~first[1:], False]                                               # the next entry belongs to the same cell
        second[:-1][nxt[:-1]] = val[csamp[1:]][nxt[:-1]]
        clear = first & ~cm.border(b)[csamp] & (second > val[csamp] * (1.0 + cm.rho) / (1.0 - cm.rho))
        pts = csamp[clear] * cm.stride
        expect[pts], decided[pts] = True, True
    return expect, decided


# ------------------------------------------------------------------------------------------------- which paths a case reaches
def zpass_form(nz, Hd, Wd):
    """(samples per block, window rows, window columns, second window) of the window z pass the product picks; None: the cache form"""
    if Wd < 128:
        return None
    return (4096, 48, 128, True) if nz >= 2 * Hd * Wd else (2048, 64, 128, False)


def window_blocks(cm, b):
    """Per block of the window form, from the float64 model: its anchor (the block's middle sample; its first in a run cut short by the
    end of the cloud), its window and how many samples fall outside.  A block counts only when its anchor is an interior sample
    (`certain`: the window is then where the model puts it); the outside count is exact up to the block's border samples (out_lo, out_hi)."""
    p, s = cm.poses[b], cm.samples()
    nz = len(p.rowf[s])
    PTS, TH, TW, _ = zpass_form(nz, cm.Hd, cm.Wd)
    cell, border = cm.cell(b), cm.border(b)
    row, col = cell // cm.Wd, cell % cm.Wd
    blocks = []
    for base in range(0, nz, PTS):
        short = base + PTS // 2 > nz - 1
        a = base if short else base + PTS // 2
        r0, c0 = int(row[a]) - TH // 2, (int(col[a]) - TW // 2) % cm.Wd
        r, c, bd = row[base:base + PTS], col[base:base + PTS], border[base:base + PTS]
        tr, tc = r - r0, (c - c0) % cm.Wd
        inside = (tr >= 0) & (tr < TH) & (tc < TW)
        out, nb = int((~inside).sum()), int(bd.sum())
        certain = not border[a]
        blocks.append(dict(certain=certain, short=short, out_lo=out - nb, out_hi=out + nb,
                           wraps=certain and c0 + TW > cm.Wd and bool((inside & ~bd & (c < c0)).any()),
                           pole=certain and (r0 < 0 or r0 + TH > cm.Hd)))
    return blocks


# ------------------------------------------------------------------------------------------------- the device side
def zbuf_offset(lib, B, Hd, Wd):
    """byte offset of the z-buffers in pcl_depth_mask's workspace, from the public size query (include/piccolo_hip.h)"""
    return lib.pcl_depth_workspace_bytes(B, Hd, Wd) - ((B * Hd * Wd * 4 + 15) & ~15)


def run_depth_mask(ops, cloud, trans, rot, grid, tau, stride):
    """pcl_depth_mask on a workspace of the caller's own (pre-filled with garbage) -> (z-buffers (B, Hd * Wd) uint32, byte mask (B, n))"""
    import ctypes
    import torch
    lib = ops._lib.load()
    trans, rot = ops._dev(trans).reshape(-1, 3), ops._dev(rot).reshape(-1, 3)
    B, (Hd, Wd) = int(trans.shape[0]), (int(grid[0]), int(grid[1]))
    nws = lib.pcl_depth_workspace_bytes(B, Hd, Wd)
    ws = torch.full((max(int(nws), 16),), 0x5A, dtype=torch.uint8, device=trans.device)
    vis = torch.empty(B, cloud.n, dtype=torch.uint8, device=trans.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                     # noqa: E731
    ops._lib.check(lib.pcl_depth_mask(ptr(cloud.data), cloud.n, ptr(trans), ptr(rot), B, Hd, Wd, float(tau), int(stride), ptr(vis), ptr(ws), nws,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pcl_depth_mask")
    off = zbuf_offset(lib, B, Hd, Wd)
    z = ws[off:off + B * Hd * Wd * 4].cpu().numpy().copy().view(np.uint32).reshape(B, Hd * Wd)
    return z, vis.cpu().numpy()


def make_cloud(ops, case, xyz, rgb):
    """-> (cloud, order): order maps packed slot -> original point"""
    import torch
    x, c = case_points(case, xyz, rgb)
    cloud = ops.Cloud(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(c)).cuda(), sort=CASES[case]["sort"])
    order = cloud.order.cpu().numpy() if cloud.order is not None else np.arange(len(x), dtype=np.int64)
    return cloud, order


def dump_cases(path):
    """Body of one child process of the cross-form comparison: every case's z-buffers, byte masks and point order into an .npz"""
    import torch
    from piccolo_amd import ops
    assert torch.cuda.is_available()
    xyz, rgb = occluder_scene()
    trans, rot = case_poses()
    out = {}
    for name, k in CASES.items():
        cloud, order = make_cloud(ops, name, xyz, rgb)
        z, vis = run_depth_mask(ops, cloud, trans, rot, k["grid"], k["tau"], k["stride"])
        out[name + "_z"], out[name + "_vis"], out[name + "_order"] = z, vis, order
    torch.cuda.synchronize()
    np.savez(path, **out)
