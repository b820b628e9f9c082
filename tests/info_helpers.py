"""The pose information matrix and covariance, in float64 from the per-point model (not a test module; tests/test_pose_information.py,
DESIGN.md section 4.1e).

info_model(): M, S1, S2, H = sum w j j^T, b = sum w l j, sigma^2 = S2 / M and cov = sigma^2 H^-1 over the pairs `sel` of a model of
grad_helpers.model (its rows `grad` and `loss`), in float64.  info_from_a(): the same through a = [g; tau] and the 6 x 6 map C of the chain
rule, H = C (sum w a a^T) C^T, the way the device forms it.

bounds(): what the device is held to on a case — the entry-wise propagation of the per-point bound test_point_gradients holds it to.
violations(): a result against those bounds; the GPU test asserts that there are none, the CPU test that every planted variant of
info_model has some.

VARIANTS: planted mistakes of info_model."""
import numpy as np

import grad_helpers as gh

U = 2.0 ** -24
CASES = ("G2", "odd", "tiny", "tall")
# fp32 roundings on the longest path of one of the kernel's 30 sums: the factor w (1), the product inside the fma and the addition to the
# lane's accumulator for each of a chunk's two steps (2), the two packed halves (1), four DPP steps inside a row of 16 lanes (4), the four
# row sums pairwise (2), the four waves' sums pairwise (2) — 12; the chunks' rows are then added in double.  One more for the output.
ADDS = 13

VARIANTS = {
    "w_squared": "(a) w^2 in place of w",
    "masked_in": "(b) masked points contribute",
    "pitch_roll": "(c) pitch and roll swapped in C",
    "tau_negated": "(d) tau negated",
    "packed_swap": "(e) two of the 21 packed entries swapped on unpacking",
    "h_over_m": "(f) H divided by M",
    "sigma_s1": "(g) sigma^2 from S1^2 / M^2 in place of S2 / M",
}


def chain_map(oracle, rot, variant=None):
    """C (6,6) float64 of pose angles rot (3,): j = C [g; tau] — grad_t = -R^T g; yaw = tau_z; pitch = -sy tau_x + cy tau_y;
    roll = cy cp tau_x + sy cp tau_y - sp tau_z"""
    R = gh.rotations(oracle, np.asarray(rot, np.float64).reshape(1, 3), np.float64)[0][0]
    y, p = float(rot[0]), float(rot[1])
    sy, cy, sp, cp = np.sin(y), np.cos(y), np.sin(p), np.cos(p)
    C = np.zeros((6, 6))
    C[:3, :3] = -R.T
    C[3, 5] = 1.0
    C[4, 3], C[4, 4] = -sy, cy
    C[5, 3], C[5, 4], C[5, 5] = cy * cp, sy * cp, -sp
    if variant == "pitch_roll":
        C[[4, 5]] = C[[5, 4]]
    if variant == "tau_negated":
        C[:, 3:] = -C[:, 3:]
    return C


def abs_terms(m64):
    """ahat (m,6) >= |a|: the model's a = [g; tau] with absolute values taken term by term, the size fp32 rounding of a is relative to.
    g = alpha grad(phi) + beta grad(theta) (alpha = -dl/dgx / pi, beta = 2 dl/dgy / pi) and tau = p x g are sums that can cancel exactly —
    a clipped azimuth leaves g along the meridian, and tau_z = px gy - py gx is 0 in exact arithmetic where the device keeps the rounding
    of its two products — so ghat = |alpha| |grad phi| + |beta| |grad theta| and tauhat_x = |py| ghat_z + |pz| ghat_y, and so on."""
    p = np.asarray(m64["p"], np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    a, b, rho = x + gh.EPS, z + gh.EPS, np.hypot(x, y)
    s1, s2 = a * a + y * y, rho * rho + b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        rx, ry = np.where(rho > 0, x / rho, 0), np.where(rho > 0, y / rho, 0)
        vp = np.abs(np.stack([-y / s1, a / s1, np.zeros_like(x)], 1))
        vt = np.abs(np.stack([b / s2 * rx, b / s2 * ry, -rho / s2], 1))
    gc = np.asarray(m64["gc"], np.float64)
    g = np.abs(gc[:, :1] / np.pi) * vp + np.abs(2 * gc[:, 1:2] / np.pi) * vt
    ap = np.abs(p)
    tau = np.stack([ap[:, 1] * g[:, 2] + ap[:, 2] * g[:, 1], ap[:, 2] * g[:, 0] + ap[:, 0] * g[:, 2], ap[:, 0] * g[:, 1] + ap[:, 1] * g[:, 0]], 1)
    return np.concatenate([g, tau], 1)


def _finish(M, S1, S2, H, b, variant=None):
    if variant == "h_over_m":
        H = H / M
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma2 = (S1 * S1) / (M * M) if variant == "sigma_s1" else S2 / M
    try:
        cov = sigma2 * np.linalg.inv(H)
    except np.linalg.LinAlgError:
        cov = np.full((6, 6), np.nan)
    return dict(M=M, S1=S1, S2=S2, H=H, b=b, sigma2=sigma2, cov=cov)


def info_model(m, sel, w, variant=None, rot=None, oracle=None, rgb=None):
    """float64 sums over the pairs sel (m,) bool of the model m with weights w (m,).  The variants that act on C or on the packed
    entries need `oracle` and the pose's angles `rot`; "masked_in" needs the points' colours `rgb` (a masked point samples exact black:
    l = ||rgb||, and its j is the model's C a)."""
    assert variant is None or variant in VARIANTS, variant
    w = np.asarray(w, np.float64)
    if variant in ("pitch_roll", "tau_negated", "packed_swap", "masked_in"):
        return info_from_a(oracle, m, sel, w, rot, variant, rgb)
    j, l = np.asarray(m["grad"], np.float64)[sel], np.asarray(m["loss"], np.float64)[sel]
    ws = w[sel] ** 2 if variant == "w_squared" else w[sel]
    H = np.einsum("i,ik,il->kl", ws, j, j)
    return _finish(ws.sum(), (ws * l).sum(), (ws * l * l).sum(), H, np.einsum("i,i,ik->k", ws, l, j), variant)


def info_from_a(oracle, m, sel, w, rot, variant=None, rgb=None):
    """the same through A = sum w a a^T (packed as the kernel packs it: 21 entries k <= l, row-major) and H = C A C^T"""
    a = np.concatenate([np.asarray(m["g"], np.float64), np.asarray(m["tau"], np.float64)], 1)
    l = np.asarray(m["loss"], np.float64).copy()
    sel = np.asarray(sel).copy()
    w = np.asarray(w, np.float64)
    if variant == "masked_in":
        extra = ~np.asarray(m["kept"]) & (w > 0)
        l[extra] = np.sqrt((np.asarray(rgb, np.float64)[extra] ** 2).sum(1))
        sel |= extra
    a, l, ws = a[sel], l[sel], w[sel]
    packed = np.array([(ws * a[:, k] * a[:, q]).sum() for k in range(6) for q in range(k, 6)])
    if variant == "packed_swap":
        packed[[2, 7]] = packed[[7, 2]]                       # (0,2) <-> (1,2)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = packed
    A = A + np.triu(A, 1).T
    C = chain_map(oracle, rot, variant)
    return _finish(ws.sum(), (ws * l).sum(), (ws * l * l).sum(), C @ A @ C.T, C @ ((ws * l) @ a))


# ------------------------------------------------------------------------------------------------------------ the device bound
_BOUNDS = {}


def bounds(oracle, name, b, flt=False, scale=1.0):
    """dict for pose b of a case: sel (the decisive kept pairs), w = scale x ok (0/1 weights for scale 1; every sum and its bound is
    linear in the scale), ref (info_model in float64), yard (info_model of the
    fp32 model's rows, summed in float64: what fp32 per-point terms give), and the entry-wise bounds BH (6,6), Bb (6,), BS1, BS2, Bsig.

    Per point the device's j is within d_i = FACTOR x (the fp32 model's worst e_i of this case and pose) x max(||j_i||inf, s) of the model's
    in every component (what test_point_gradients asserts, s the median of ||j_i||inf), and its l within e = FACTOR x (the fp32 model's
    worst |l32 - l64|) (what the residual test asserts).  So, with the kernel's ADDS fp32 roundings per sum,
      |H_kl - H64_kl| <= sum_i (|j_ik| d_i + |j_il| d_i + d_i^2) + ADDS u sum_i |j_ik j_il|
      |b_k - b64_k|   <= sum_i (l_i d_i + |j_ik| e + d_i e) + ADDS u sum_i l_i |j_ik|
      |S1 - S1_64|    <= n e + ADDS u S1          |S2 - S2_64| <= sum_i (2 l_i e + e^2) + ADDS u S2
      |sigma^2 - sigma^2_64| <= BS2 / M + 2 u sigma^2      (M is exact: one division in double, one rounding)"""
    key = (name, b, flt, scale)
    if key in _BOUNDS:
        return _BOUNDS[key]
    m64, m32, ok, _, _ = gh.case_rule(oracle, name, b, flt)
    sel = ok & m64["kept"]
    w = scale * ok.astype(np.float64)
    ref = info_model(m64, sel, w)
    m32d = dict(grad=m32["grad"].astype(np.float64), loss=m32["loss"].astype(np.float64))
    yard = info_model(m32d, sel, w)
    j, l = np.abs(m64["grad"][sel]), m64["loss"][sel]
    rn = j.max(1)
    s = max(float(np.median(rn)), 1e-300)
    worst = gh.three_stats(gh.point_errors(m32["grad"], m64["grad"], sel))[2]
    d = gh.FACTOR * worst * np.maximum(rn, s)
    e = gh.FACTOR * float(np.abs(m32["loss"].astype(np.float64) - m64["loss"])[sel].max())
    jd = (j * d[:, None]).sum(0)
    BH = scale * (jd[:, None] + jd[None, :] + (d * d).sum() + ADDS * U * np.einsum("ik,il->kl", j, j))
    Bb = scale * ((l * d).sum() + e * j.sum(0) + e * d.sum() + ADDS * U * (l[:, None] * j).sum(0))
    BS1 = scale * len(l) * e + ADDS * U * ref["S1"]
    BS2 = scale * (2 * l * e + e * e).sum() + ADDS * U * ref["S2"]
    out = dict(sel=sel, w=w, ref=ref, yard=yard, BH=BH, Bb=Bb, BS1=BS1, BS2=BS2, Bsig=BS2 / ref["M"] + 2 * U * ref["sigma2"], worst=worst,
               rot=gh.scene(oracle, name)[5][b], rgb=gh.scene(oracle, name)[1], m64=m64)
    _BOUNDS[key] = out
    return out


def cov_bound(H, cov):
    """||cov_dev - sigma^2 inv(H)||_F <= 20 cond(H) 2^-24 ||cov||_F for cov_dev formed in double from the exact double H~ whose rounding to
    fp32 is `H`, sigma^2 likewise: the fp32 H and sigma^2 the comparison starts from are within 2^-24 of H~ and sigma~^2 entry by entry
    (relative perturbation of the inverse <= cond x ||dH|| / ||H|| <= cond x 2^-24 x sqrt(6) at most for Frobenius against 2-norm:
    2.5), the Cholesky inverse in double adds cond x 2^-52 x small (nothing at this scale), sigma^2's rounding 2^-24 and the output's
    rounding 2^-24 (cond >= 1): 2.5 + 1 + 1 = 4.5, taken as 20 for the slack between norms of a 6 x 6 matrix."""
    return 20.0 * np.linalg.cond(H) * U * np.linalg.norm(cov)


def violations(got, bd):
    """-> list of (quantity, achieved / bound) with achieved > bound, of a result dict `got` (M, S1, S2, H, b, sigma2, cov) against bounds()
    of the same case: M exactly, S1, S2, sigma^2, every entry of H and b, and cov against sigma^2 inv(H) formed from got's own H and sigma^2"""
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
    entry("S2", got["S2"], ref["S2"], bd["BS2"])
    entry("sigma2", got["sigma2"], ref["sigma2"], bd["Bsig"])
    entry("H", got["H"], ref["H"], bd["BH"])
    entry("b", got["b"], ref["b"], bd["Bb"])
    H = np.asarray(got["H"], np.float64)
    try:
        with np.errstate(invalid="ignore"):
            want = float(got["sigma2"]) * np.linalg.inv(H)
            q = np.linalg.norm(np.asarray(got["cov"], np.float64) - want) / cov_bound(H, want)
    except np.linalg.LinAlgError:
        q = float("inf")
    if not q <= 1:
        bad.append(("cov", float(q)))
    return bad
