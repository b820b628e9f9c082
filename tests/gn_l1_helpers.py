"""The Huber-L1 form of the Levenberg-Marquardt polish in float64 (not a test module; tests/test_gn_l1_model.py, tests/test_gn_l1.py,
DESIGN.md section 4.1i).  Per kept point with residual l >= 0 and delta > 0

    phi(l) = min(1 / l, 1 / delta)        rho(l) = l - delta / 2  (l >= delta),  l^2 / (2 delta)  (l < delta)
    M = sum w m    S1 = sum w m l (both PLAIN)    S_rho = sum w m rho    F_rho = S_rho / M
    H_rho = sum w m phi j j^T    b_rho = sum w m phi l j

l1_sums(): those sums from per-point rows j, l and weights w.  evaluate_l1(): gn_helpers.evaluate's dict layout from them (S2 := S_rho,
F := float32(S_rho / M)), so that gn_helpers.lm and gn_helpers.trace_violations apply to it unchanged.

bounds_l1(): what the device's record is held to on a case — info_helpers.bounds' propagation with the weights w phi, plus the per-term
contribution of phi's own error.  violations_l1(): a record against those bounds.  device_restatement(): the pass's arithmetic in fp32 numpy
on the fp32 model's rows.

VARIANTS: planted mistakes of l1_sums."""
import numpy as np

import gn_helpers as gn
import grad_helpers as gh
import info_helpers as ih

U = ih.U
F32 = np.float32
ADDS = ih.ADDS + 2          # the pass's roundings per sum (info_helpers.ADDS) and two more: v_rcp_f32's result and the product w phi
DELTAS = (1.0 / 64, 1.0 / 255)
DELTA_SMALL = 2.0 ** -12    # below every kept residual of the eight (case, pose) pairs (the smallest is 1.0e-3)
DELTA_SATURATED = 2.0       # above every residual (they never exceed sqrt(3); the largest here is 1.53)

VARIANTS = {
    "phi_squared": "(a) phi^2 in place of phi",
    "no_floor": "(b) 1 / l without the floor at delta",
    "m_phi": "(c) M multiplied by phi",
    "s1_phi": "(d) S1 multiplied by phi",
    "rho_no_offset": "(e) rho without the - delta / 2 (discontinuous at delta)",
    "rho_no_half": "(f) l^2 / delta below delta, the factor 1 / 2 missing",
    "b_phi_twice": "(g) phi applied to b twice",
}


def phi_of(l, delta):
    with np.errstate(divide="ignore"):
        return np.minimum(1.0 / np.asarray(l, np.float64), 1.0 / delta)


def rho_of(l, delta, variant=None):
    l = np.asarray(l, np.float64)
    hi = l if variant == "rho_no_offset" else l - delta / 2
    lo = l * l / delta if variant == "rho_no_half" else l * l / (2 * delta)
    return np.where(l >= delta, hi, lo)


def l1_sums(j, l, w, delta, variant=None):
    """float64 sums over per-point rows j (m,6), l (m,), w (m,) -> dict M, S1, S2 (:= S_rho), H, b, sigma2 (:= F_rho in float64)"""
    assert variant is None or variant in VARIANTS, variant
    j, l, w, delta = np.asarray(j, np.float64), np.asarray(l, np.float64), np.asarray(w, np.float64), float(delta)
    with np.errstate(divide="ignore"):
        phi = 1.0 / l if variant == "no_floor" else phi_of(l, delta)
    ph = phi * phi if variant == "phi_squared" else phi
    H = np.einsum("i,ik,il->kl", w * ph, j, j)
    b = np.einsum("i,i,ik->k", w * (ph * phi if variant == "b_phi_twice" else ph), l, j)
    M = (w * phi).sum() if variant == "m_phi" else w.sum()
    S1 = (w * phi * l).sum() if variant == "s1_phi" else (w * l).sum()
    S2 = (w * rho_of(l, delta, variant)).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma2 = S2 / M
    return dict(M=M, S1=S1, S2=S2, H=H, b=b, sigma2=sigma2)


def evaluate_l1(oracle, scn, theta, delta, w=None, variant=None):
    """gn_helpers.evaluate for the L1 form: the sums of pose theta (6,) (fp32 values) over every kept pair of the scene scn = (xyz, rgb, img),
    weights w (n,) or 1 -> dict M, S1, S2 := S_rho, H := H_rho, b := b_rho in float64, F = (float)(S_rho / M), F1 = (float)(S1 / M), ok"""
    xyz, rgb, img = scn
    theta = np.asarray(theta, F32)
    m = gh.model(oracle, xyz, rgb, img, theta[:3], theta[3:], np.float64)
    w = np.ones(len(xyz)) if w is None else np.asarray(w, np.float64)
    sel = m["kept"] & (w > 0)
    r = l1_sums(m["grad"][sel], m["loss"][sel], w[sel], delta, variant)
    with np.errstate(divide="ignore", invalid="ignore"):
        r["F"] = F32(r["S2"] / r["M"])
        r["F1"] = F32(r["S1"] / r["M"])
    r["ok"] = bool(r["M"] > 0 and np.isfinite(r["H"]).all() and np.isfinite(r["b"]).all() and np.isfinite([r["S1"], r["S2"]]).all())
    return r


_EVALUATORS = {}


def scene_evaluator_l1(oracle, name, delta, w=None, variant=None):
    """theta -> evaluate_l1() on a case's scene (its k/255 image), memoised per pose (gn_helpers.scene_evaluator's twin)"""
    key = (name, float(delta), None if w is None else np.asarray(w, F32).tobytes(), variant)
    if key not in _EVALUATORS:
        xyz, rgb, img = gh.scene(oracle, name)[:3]
        seen = {}

        def ev(theta):
            k = np.asarray(theta, F32).tobytes()
            if k not in seen:
                seen[k] = evaluate_l1(oracle, (xyz, rgb, img), theta, delta, w, variant)
            return seen[k]
        _EVALUATORS[key] = ev
    return _EVALUATORS[key]


# ------------------------------------------------------------------------------------------------------------ the device bound
_BOUNDS = {}


def case_weights(oracle, name, b, plane=None, flt=False):
    """(n,) float64 weights of a bounded comparison: ok (the decisive pairs of pose b: no border pair enters a sum, as in
    test_pose_information) times the plane (n,) where there is one"""
    ok = gh.case_rule(oracle, name, b, flt)[2]
    return ok.astype(np.float64) * (1.0 if plane is None else np.asarray(plane, np.float64))


def bounds_l1(oracle, name, b, delta, plane=None, flt=False, variant=None):
    """dict for pose b of a case under the weights case_weights(plane): sel, w, ref (l1_sums in float64), and the entry-wise bounds BH
    (6,6), Bb (6,), BS1, BS2 (of S_rho), Bsig (of F_rho).

    info_helpers.bounds' propagation with the weights w phi.  Per point the device's j is within d_i of the model's in every component
    and its l within e (info_helpers.bounds: what test_point_gradients and the residual test assert).  Its phi is v_rcp_f32 of its own l,
    cut at the host's 1 / delta:  |phi^ - phi| <= phi (e / max(l, delta) + 2 u) =: f_i  (d(1/l) = e / l^2 = phi e / l above delta, nothing
    below it; one rounding for the reciprocal, one for w phi).  So, with ADDS = info_helpers.ADDS + 2 fp32 roundings per sum,
      |H_kl - H64_kl| <= sum_i w_i [f_i |j_ik j_il| + (phi_i + f_i) (|j_ik| d_i + |j_il| d_i + d_i^2)] + ADDS u sum_i w_i phi_i |j_ik j_il|
      |b_k - b64_k|   <= sum_i w_i [f_i l_i |j_ik| + (phi_i + f_i) (l_i d_i + |j_ik| e + d_i e)] + ADDS u sum_i w_i phi_i l_i |j_ik|
      |S1 - S1_64|    <= sum_i w_i e + info_helpers.ADDS u S1                       (plain: the L2 pass's own bound)
      |S_rho - S_rho64| <= sum_i w_i e min(1, (l_i + e) / delta) + ADDS u S_rho     (rho' = phi l <= min(1, l / delta))
      |F_rho - F_rho64| <= BS_rho / M + 2 u F_rho                                   (M is exact)"""
    key = (name, b, float(delta), None if plane is None else np.asarray(plane, F32).tobytes(), flt)
    if key not in _BOUNDS:
        m64, m32, ok, _, _ = gh.case_rule(oracle, name, b, flt)
        sel = ok & m64["kept"]
        wf = case_weights(oracle, name, b, plane, flt)
        w = wf[sel]
        ref = l1_sums(m64["grad"][sel], m64["loss"][sel], w, delta)
        j, l = np.abs(m64["grad"][sel]), m64["loss"][sel]
        rn = j.max(1)
        s = max(float(np.median(rn)), 1e-300)
        worst = gh.three_stats(gh.point_errors(m32["grad"], m64["grad"], sel))[2]
        d = gh.FACTOR * worst * np.maximum(rn, s)
        e = gh.FACTOR * float(np.abs(m32["loss"].astype(np.float64) - m64["loss"])[sel].max())
        phi = phi_of(l, delta)
        f = phi * (e / np.maximum(l, delta) + 2 * U)
        jj = np.einsum("ik,il->ikl", j, j)
        jd = j * d[:, None]
        BH = (np.einsum("i,ikl->kl", w * f, jj) + np.einsum("i,ikl->kl", w * (phi + f), jd[:, :, None] + jd[:, None, :] + (d * d)[:, None, None])
              + ADDS * U * np.einsum("i,ikl->kl", w * phi, jj))
        Bb = ((w * f * l) @ j + (w * (phi + f)) @ (l[:, None] * d[:, None] + e * j + (e * d)[:, None]) + ADDS * U * ((w * phi * l) @ j))
        BS1 = (w * e).sum() + ih.ADDS * U * ref["S1"]
        BS2 = (w * e * np.minimum(1.0, (l + e) / delta)).sum() + ADDS * U * ref["S2"]
        _BOUNDS[key] = dict(sel=sel, w=wf, ref=ref, BH=BH, Bb=Bb, BS1=BS1, BS2=BS2, Bsig=BS2 / ref["M"] + 2 * U * ref["sigma2"], m64=m64, m32=m32,
                            e=e, rot=gh.scene(oracle, name)[5][b])
    bd = _BOUNDS[key]
    if variant is not None:
        m64, sel = bd["m64"], bd["sel"]
        return dict(bd, got=l1_sums(m64["grad"][sel], m64["loss"][sel], bd["w"][sel], delta, variant))
    return bd


def violations_l1(got, bd):
    """-> list of (quantity, achieved / bound) with achieved > bound, of a record `got` (M, S1, S2 := S_rho, sigma2 := F_rho, H, b) against
    bounds_l1 of the same case: M exactly, the rest entry by entry"""
    ref, bad = bd["ref"], []
    if got["M"] != ref["M"]:
        bad.append(("M", float("inf")))

    def entry(name, a, r, B):
        with np.errstate(invalid="ignore"):
            q = np.abs(np.asarray(a, np.float64) - r) / B
        q = np.where(np.isfinite(q), q, np.inf)
        if (q > 1).any():
            bad.append((name, float(q.max())))
    entry("S1", got["S1"], ref["S1"], bd["BS1"])
    entry("S_rho", got["S2"], ref["S2"], bd["BS2"])
    entry("F_rho", got["sigma2"], ref["sigma2"], bd["Bsig"])
    entry("H", got["H"], ref["H"], bd["BH"])
    entry("b", got["b"], ref["b"], bd["Bb"])
    return bad


def _sum32(x):
    """fp32 sum of the rows of x in fp32, pairwise (numpy's order: another order than the device's, the same format)"""
    return np.add.reduce(np.asarray(x, F32), axis=0, dtype=F32)


def device_restatement(oracle, bd, delta):
    """The pass's arithmetic in fp32 numpy on the fp32 model's rows of bounds_l1's case: phi = min(1 / l, 1 / delta) in fp32 with the host's
    fp32 1 / delta, wp = w phi, wa = wp a, the 21 + 6 sums of (wa_k) a_l and (wa_k) l, w rho with rho = l >= delta ? l - delta / 2 :
    l l (0.5 / delta), w l and w — every product and sum rounded to fp32 —, then the chain rule H = C A C^T, b = C v in double.
    -> a record in violations_l1's layout"""
    m32, sel = bd["m32"], bd["sel"]
    a = np.concatenate([m32["g"], m32["tau"]], 1).astype(F32)[sel]
    l = m32["loss"].astype(F32)[sel]
    w = bd["w"][sel].astype(F32)
    inv_delta, half_delta = F32(1) / F32(delta), F32(0.5) * F32(delta)
    with np.errstate(divide="ignore"):
        phi = np.minimum(F32(1) / l, inv_delta).astype(F32)
    wa = ((w * phi).astype(F32)[:, None] * a).astype(F32)
    packed = np.array([_sum32(wa[:, k] * a[:, q]) for k in range(6) for q in range(k, 6)], np.float64)
    v = np.array([_sum32(wa[:, k] * l) for k in range(6)], np.float64)
    d = half_delta + half_delta
    rho = np.where(l >= d, l - half_delta, ((l * l).astype(F32) * (F32(0.5) * inv_delta)).astype(F32)).astype(F32)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = packed
    A = A + np.triu(A, 1).T
    C = ih.chain_map(oracle, bd["rot"])
    M, S1, S2 = float(_sum32(w)), float(_sum32(w * l)), float(_sum32(w * rho))
    return dict(M=M, S1=float(F32(S1)), S2=float(F32(S2)), sigma2=float(F32(S2 / M)), H=(C @ A @ C.T).astype(F32).astype(np.float64),
                b=(C @ v).astype(F32).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------- the free run
_FREE = {}


def free_centre(oracle, name, delta):
    """(theta, F_rho) the L1 model converges to from pose 1 of the case's scene: 40 iterations of gn_helpers.lm with the defaults"""
    if ("centre", name, delta) not in _FREE:
        r = gn.lm(scene_evaluator_l1(oracle, name, delta), gn.scene_pose(oracle, name, 1), 40, gn.hyper())
        _FREE["centre", name, delta] = (r["theta"], r["sigma2"])
    return _FREE["centre", name, delta]


def free_starts(oracle, name, delta):
    """the starts of the free-run test: the L1 model's converged pose + gn_helpers.FREE_OFFSETS, in fp32"""
    return [(free_centre(oracle, name, delta)[0].astype(np.float64) + off).astype(F32) for off in gn.FREE_OFFSETS]


def free_yardstick(oracle, name, delta, i):
    """gn_helpers.free_yardstick with evaluate_l1 as the model: (lo, hi, own) of the final F_rho after gn_helpers.FREE_ITERS iterations from
    start i and its 12 one-ulp neighbours"""
    if ("yard", name, delta, i) not in _FREE:
        ev, start, h = scene_evaluator_l1(oracle, name, delta), free_starts(oracle, name, delta)[i], gn.hyper()
        finals = [float(gn.lm(ev, start, gn.FREE_ITERS, h)["sigma2"])]
        for c in range(6):
            for to in (-np.inf, np.inf):
                s = start.copy()
                s[c] = np.nextafter(s[c], F32(to))
                finals.append(float(gn.lm(ev, s, gn.FREE_ITERS, h)["sigma2"]))
        _FREE["yard", name, delta, i] = (min(finals), max(finals), finals[0])
    return _FREE["yard", name, delta, i]
