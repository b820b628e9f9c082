"""Pose information, residuals and the LM chain UNDER THE DEPTH MASK, composed in float64 from the models the plain forms are tested with
(not a test module; tests/test_depth_info_model.py, tests/test_depth_info.py):

    depth_helpers.CaseModel / expected_visible      which points a z-buffer hides, and which of them the model can decide
    grad_helpers.model                              the per-point terms l, j of every (point, pose) pair
    info_helpers.info_model / violations            the sums M, S1, S2, H, b, sigma^2, cov over a set of pairs, and the bound check
    gn_helpers.lm                                   the LM chain on an evaluation function

The masked sums of a pose are info_model over the pairs that are kept (not black) AND visible: 0/1 weights.  The visibility comes from a
z-buffer — the model's own (reference_zbuffer) on the CPU, the device's row on the GPU.

BOUNDS.  info_helpers.bounds is keyed by the names of grad_helpers' scenes and lets only DECISIVE pairs into a sum through a weight plane.
Under the mask a weighted cloud is refused, so every visible kept pair enters the device's sums, the border pairs among them.  bounds()
below restates info_helpers.bounds' formulas for any scene and any 0/1 selection, with
  * `worst` and the loss error e taken over the decisive pairs of the selection (as there), applied to every pair of it, and
  * an allowance for the selection's border pairs (a pixel coordinate within 3 x the model's own fp32-vs-fp64 gap of a texel border or of
    the clip, grad_helpers.decisive): fp32 may evaluate such a pair in the neighbouring texel cell.  The bilinear colour is continuous
    across the border, so l moves by rounding only; j is that cell's.  The allowance takes the neighbour's |j| component-wise no larger
    than twice the pair's own (ASSUMPTION, stated here; the pairs concerned are under grad_helpers.BORDER_CAP of a case):
        H_kl: + sum_border 2 (2 |j_ik| |j_il|)          b_k: + sum_border 2 l_i |j_ik|
A pair whose black decision differs between the fp64 and the fp32 model is never decisive; bounds() reports how many such pairs the
selection holds (`undecided_kept`) and the tests require 0 of them to be visible on their cases."""
import numpy as np

import depth_helpers as dh
import gn_helpers as gn
import grad_helpers as gh
import info_helpers as ih

H, W = 128, 256
TINY_GRID = (16, 32)
# name -> (points used (None: all), grid, stride, tau): depth_helpers' W1 / W4 / W7 / C1 and two tiny clouds on a 16 x 32 grid — 513: one
# chunk of two steps, the second holding one point; 700: a last step cut short
CASES = {name: (None, dh.CASES[name]["grid"], dh.CASES[name]["stride"], dh.CASES[name]["tau"]) for name in ("W1", "W4", "W7", "C1")}
CASES.update({"t513": (513, TINY_GRID, 1, 0.0), "t700": (700, TINY_GRID, 1, 0.0)})
NOTHING_HIDDEN_TAU = 1e6

_SCENE = {}


def scene(oracle):
    """(xyz, rgb, img k/255 (H, W, 3), trans (3,3), rot (3,3)): depth_helpers' occluder scene and poses, the panorama rendered as
    test_zpass_exact renders it"""
    if not _SCENE:
        from piccolo_amd import synth
        xyz, rgb = dh.occluder_scene()
        trans, rot = dh.case_poses()
        t_gt, ypr_gt = synth.gt_pose(17)
        img = oracle.make_pano_u8(synth.transform_cloud(xyz, t_gt, ypr_gt), rgb, (H, W)).astype(np.float32) / 255
        _SCENE["s"] = (xyz, rgb, img, np.asarray(trans, np.float32), np.asarray(rot, np.float32))
    return _SCENE["s"]


def case_points(case, xyz, rgb):
    k = CASES[case][0]
    return (xyz, rgb) if k is None else (xyz[:k], rgb[:k])


def depth_kw(case):
    _, grid, stride, tau = CASES[case]
    return {"depth_res": grid, "depth_tau": tau, "depth_stride": stride}


def case_model(oracle, case, order, tau=None, poses=None):
    """depth_helpers.CaseModel of a case in the point order `order` (packed slot -> point)"""
    xyz, rgb, _, trans, rot = scene(oracle)
    _, grid, stride, tau0 = CASES[case]
    x = case_points(case, xyz, rgb)[0][order]
    trans, rot = (trans, rot) if poses is None else poses
    return dh.CaseModel(x, trans, rot, grid, stride, tau0 if tau is None else tau)


_MODELS = {}


def point_models(oracle, b):
    """(m64, m32) of grad_helpers.model for EVERY point of the scene at pose b, in the scene's own order (a case takes rows of it)"""
    if b not in _MODELS:
        xyz, rgb, img, trans, rot = scene(oracle)
        _MODELS[b] = tuple(gh.model(oracle, xyz, rgb, img, trans[b], rot[b], dt) for dt in (np.float64, np.float32))
    return _MODELS[b]


def take(m, idx):
    return {key: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == len(m["kept"]) else v) for key, v in m.items()}


def masked_info(m64, visible):
    """info_model over the kept pairs with the 0/1 weights `visible` — M, S1, S2, H, b, sigma2, cov in float64"""
    vis = np.asarray(visible).astype(bool)
    return ih.info_model(m64, m64["kept"] & vis, vis.astype(np.float64))


def bounds(m64, m32, visible):
    """info_helpers.bounds' dict (ref, yard, BH, Bb, BS1, BS2, Bsig, worst) for the model rows m64 / m32 (same points, same pose) and the
    0/1 selection `visible`, plus border_share and undecided_kept (module docstring)"""
    vis = np.asarray(visible).astype(bool)
    ok = gh.decisive(m64, m32)[0]
    sel = m64["kept"] & vis
    dec = sel & ok
    w = vis.astype(np.float64)
    ref = ih.info_model(m64, sel, w)
    both = sel & m32["kept"]
    yard = ih.info_model(dict(grad=m32["grad"].astype(np.float64), loss=m32["loss"].astype(np.float64)), both, w)
    j, l = np.abs(m64["grad"][sel]), m64["loss"][sel]
    rn = j.max(1)
    s = max(float(np.median(rn)), 1e-300)
    worst = gh.three_stats(gh.point_errors(m32["grad"], m64["grad"], dec))[2]
    d = gh.FACTOR * worst * np.maximum(rn, s)
    e = gh.FACTOR * float(np.abs(m32["loss"].astype(np.float64) - m64["loss"])[dec].max())
    jd = (j * d[:, None]).sum(0)
    border = ~ok[sel]
    jb, lb = j[border], l[border]
    BH = jd[:, None] + jd[None, :] + (d * d).sum() + ih.ADDS * ih.U * np.einsum("ik,il->kl", j, j) + 4.0 * np.einsum("ik,il->kl", jb, jb)
    Bb = (l * d).sum() + e * j.sum(0) + e * d.sum() + ih.ADDS * ih.U * (l[:, None] * j).sum(0) + 2.0 * (lb[:, None] * jb).sum(0)
    BS1 = len(l) * e + ih.ADDS * ih.U * ref["S1"]
    BS2 = (2 * l * e + e * e).sum() + ih.ADDS * ih.U * ref["S2"]
    return dict(sel=sel, w=w, ref=ref, yard=yard, BH=BH, Bb=Bb, BS1=BS1, BS2=BS2, Bsig=BS2 / ref["M"] + 2 * ih.U * ref["sigma2"], worst=worst,
                border_share=float(border.mean()) if len(border) else 0.0, undecided_kept=int((vis & (m64["kept"] != m32["kept"])).sum()))


def masked_evaluator(oracle, case, order, b_unused=None):
    """ev(theta) for gn_helpers.lm on a case: the sums of gn_helpers.evaluate over the pairs the MODEL'S OWN z-buffer at theta keeps
    (reference_zbuffer of a one-pose CaseModel at theta, visible = d2 <= Z[cell] in float64 — the objective is rebuilt at every pose)"""
    xyz, rgb, img, _, _ = scene(oracle)
    x, c = case_points(case, xyz, rgb)
    x, c = x[order], c[order]
    _, grid, stride, tau = CASES[case]

    def ev(theta):
        theta = np.asarray(theta, np.float32)
        cm = dh.CaseModel(x, theta[None, :3], theta[None, 3:], grid, stride, tau)
        z = np.full(cm.Hd * cm.Wd, np.inf)                                     # (reference_zbuffer before its rounding to fp32 words)
        np.minimum.at(z, cm.cell(0), cm.poses[0].val[cm.samples()])
        vis = cm.poses[0].d2 <= z[cm.cell(0, slice(None))]
        return gn.evaluate(oracle, (x, c, img), theta, w=vis.astype(np.float64))
    return ev
