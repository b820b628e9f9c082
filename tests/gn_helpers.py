"""The Levenberg-Marquardt pose polish in float64 with its decisions in fp32 (not a test module; tests/test_gn_model.py,
tests/test_gn_refine.py).

evaluate(): M, S1, S2, H, b of one pose over every kept pair of a scene — grad_helpers.model in float64 and info_helpers.info_model.
lm(): the chain pcl_gn_refine runs, on such evaluations: evaluation k = 0 .. iters at theta_try, accept iff the sums are finite, M > 0 and
(float)(S2 / M) < F_acc in fp32 (k = 0: iff finite and M > 0), lambda x lam_down on acceptance (not at k = 0) and x lam_up on rejection
in fp32 with the clamps, the step (H + lambda diag H) delta = -b on the ACCEPTED sums in double, the whole delta scaled to the cap, theta_try =
(float)((double)theta_acc + delta).  Its result has the layout of the device's: out fields, a trace of (iters + 1, 16) float32 rows.

trace_violations(): what the GPU test asserts of a device run, written once so that the CPU test can apply it to lm() with a planted
mistake switched on.  `info_at(theta)` is the yardstick evaluation of a pose: ops.pose_information for the device, evaluate() for the model.

VARIANTS: planted mistakes of lm()."""
import numpy as np

import grad_helpers as gh
import info_helpers as ih

U = ih.U
F32 = np.float32
HYPER = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)
TRACE_ROW = 16                        # theta_try (6), F, accepted, lambda after the decision, M, 0 x 6

VARIANTS = {
    "step_sign": "(a) the step has the wrong sign",
    "lam_identity": "(b) lambda I in place of lambda diag H",
    "accept_le": "(c) <= in place of < in the acceptance",
    "lam_not_raised": "(d) lambda is not raised on rejection",
    "lam_down_at_0": "(e) lambda is lowered at k = 0",
    "cap_per_component": "(f) the cap clips every component instead of scaling delta",
    "solve_on_trial": "(g) the solve runs on the rejected trial's H and b instead of the accepted ones",
    "f_from_s1": "(h) S1 / M in place of S2 / M",
}


def hyper(**kw):
    h = dict(HYPER)
    for key, v in kw.items():
        assert key in h, key
        h[key] = v
    return {key: F32(v) for key, v in h.items()}


def evaluate(oracle, scn, theta, w=None):
    """the sums of pose theta (6,) (fp32 values) over the scene scn = (xyz, rgb, img): every kept pair, weights w (n,) or 1 -> dict with
    M, S1, S2, H, b, sigma2, cov in float64, F = (float)(S2 / M), ok (sums finite and M > 0)"""
    xyz, rgb, img = scn
    theta = np.asarray(theta, F32)
    m = gh.model(oracle, xyz, rgb, img, theta[:3], theta[3:], np.float64)
    sel = m["kept"]
    w = np.ones(len(xyz)) if w is None else np.asarray(w, np.float64)
    sel = sel & (w > 0)
    r = ih.info_model(m, sel, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        r["F"] = F32(r["S2"] / r["M"])
        r["F1"] = F32(r["S1"] / r["M"])
    r["ok"] = bool(r["M"] > 0 and np.isfinite(r["H"]).all() and np.isfinite(r["b"]).all() and np.isfinite([r["S1"], r["S2"]]).all())
    return r


def solve_step(H, b, lam, cap, variant=None):
    """delta (6,) float64 of (H + lam diag H) delta = -b, the whole of it scaled to max |delta_i| = cap where that is exceeded; None where
    the damped matrix has no Cholesky factor"""
    H, b, lam = np.asarray(H, np.float64), np.asarray(b, np.float64), float(lam)
    D = H + lam * (np.eye(6) if variant == "lam_identity" else np.diag(np.diag(H)))
    try:
        np.linalg.cholesky(D)
    except np.linalg.LinAlgError:
        return None
    d = np.linalg.solve(D, b if variant == "step_sign" else -b)
    mx, cap = np.abs(d).max(), float(cap)
    if mx > cap:
        d = np.clip(d, -cap, cap) if variant == "cap_per_component" else d * (cap / mx)
    return d


def lam_next(lam, accepted, k, h, variant=None):
    """the fp32 recurrence of lambda after the decision of evaluation k"""
    lam = F32(lam)
    if accepted:
        if k > 0 or variant == "lam_down_at_0":
            lam = max(F32(lam * h["lam_down"]), h["lam_min"])
    elif variant != "lam_not_raised":
        lam = min(F32(lam * h["lam_up"]), h["lam_max"])
    return F32(lam)


def lm(ev, theta0, iters, h, variant=None):
    """the chain on the evaluation function ev(theta) -> evaluate()'s dict -> dict(theta, sigma2_start, sigma2, lam, accepted, rejected,
    evaluations, status, trace (iters + 1, 16) float32, sums: the accepted evaluation)"""
    assert variant is None or variant in VARIANTS, variant
    acc = np.asarray(theta0, F32).copy()
    tri = acc.copy()
    F_acc, F_start, lam = F32(np.inf), F32(np.nan), F32(h["lam0"])
    n_acc = n_rej = n_ev = status = 0
    sums = solve_on = None
    trace = np.zeros((iters + 1, TRACE_ROW), F32)
    for k in range(iters + 1):
        r = ev(tri)
        F = r["F1"] if variant == "f_from_s1" else r["F"]
        n_ev += 1
        if k == 0:
            ok = r["ok"]
        else:
            ok = r["ok"] and bool(F <= F_acc if variant == "accept_le" else F < F_acc)
        if ok:
            acc, F_acc, sums, solve_on = tri.copy(), F, r, r
            n_acc += 1
            if k == 0:
                F_start = F
        else:
            n_rej += 1
            if variant == "solve_on_trial":
                solve_on = r
        lam = lam_next(lam, ok, k, h, variant)
        trace[k, :6], trace[k, 6], trace[k, 7], trace[k, 8], trace[k, 9] = tri, F, float(ok), lam, F32(r["M"])
        if k == 0 and not ok:
            status, sums = 1, r
            break
        if k == iters:
            break
        d = solve_step(solve_on["H"], solve_on["b"], lam, h["step_cap"], variant)
        if d is None:
            status = 2
            break
        tri = (acc.astype(np.float64) + d).astype(F32)
        if np.abs(d).max() <= h["tol"] or np.array_equal(tri, acc):
            status = 3
            break
    return dict(theta=acc, sigma2_start=F_start, sigma2=F_acc, lam=lam, accepted=n_acc, rejected=n_rej, evaluations=n_ev, status=status,
                trace=trace, sums=sums)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)


def step_bound(H, lam, delta, theta):
    """20 cond(H + lam diag H) 2^-24 ||delta||inf + ulp(theta), per component: info_helpers.cov_bound's argument applied to a solve — the
    fp32 H and b the comparison starts from are within 2^-24 of the double ones the device solves on, entry by entry, a relative
    perturbation of the solution of at most cond x (2.5 + 1) x 2^-24; scaling to the cap divides by a maximum with the same relative
    error (x 2), the constant 20 is cov_bound's; and theta_try is rounded once to fp32."""
    H = np.asarray(H, np.float64)
    D = H + float(lam) * np.diag(np.diag(H))
    return 20.0 * np.linalg.cond(D) * U * np.abs(delta).max() + ulp32(theta)


def trace_violations(run, h, iters, info_at, report=None):
    """-> list of strings, one per broken check, of a run (lm()'s dict layout; for the device the same fields read back) under the
    hyper-parameters h: per evaluation F and M against info_at(theta_try) bit for bit; the accepted flags against the fp32 rule applied to
    the trace's own F; the lambda column against the fp32 recurrence; the counters against the flags; the returned pose, sigma2_start and
    sigma2 against the trace; every step theta_try(k + 1) - theta_acc(k) against the float64 solve on info_at(theta_acc(k))'s H and b
    within step_bound.  report(name, achieved, bound): called for the worst step."""
    bad, tr = [], np.asarray(run["trace"], F32)
    n_ev = int(run["evaluations"])
    if not 1 <= n_ev <= iters + 1:
        return ["evaluations %d outside 1 .. %d" % (n_ev, iters + 1)]
    if tr[n_ev:].any():
        bad.append("trace rows past the last evaluation are not zero")
    F_acc, lam, acc, acc_info = F32(np.inf), F32(h["lam0"]), None, None
    n_acc = n_rej = 0
    worst = (0.0, 0.0, 1.0)
    for k in range(n_ev):
        tri, F, flag, lam_k, M = tr[k, :6], tr[k, 6], tr[k, 7], tr[k, 8], tr[k, 9]
        ref = info_at(tri)
        if not np.array_equal(_bits(F), _bits(ref["F"])) or not np.array_equal(_bits(M), _bits(F32(ref["M"]))):
            bad.append("evaluation %d: F %r M %r, at that pose %r %r" % (k, F, M, ref["F"], F32(ref["M"])))
        if k > 0:
            # the step that led here, from the accepted pose and lambda after evaluation k - 1
            d = solve_step(acc_info["H"], acc_info["b"], lam, h["step_cap"])
            if d is None:
                bad.append("evaluation %d follows a damped matrix without a factor" % k)
            else:
                err = np.abs((tri.astype(np.float64) - acc.astype(np.float64)) - d)
                bound = step_bound(acc_info["H"], lam, d, np.maximum(np.abs(tri), np.abs(acc)))
                q = float((err / bound).max())
                if q >= worst[1]:
                    at = int(np.argmax(err / bound))
                    worst = (float(err[at]), q, float(bound[at]))
                if q > 1:
                    bad.append("step into evaluation %d: %.3g of the bound" % (k, q))
        want = bool(ref["ok"]) if k == 0 else bool(ref["ok"] and F < F_acc)
        if bool(flag) != want or flag not in (0.0, 1.0):
            bad.append("evaluation %d: accepted %r, the rule gives %r (F %r against %r)" % (k, flag, want, F, F_acc))
        if flag:
            acc, F_acc, acc_info = tri.copy(), F, ref
            n_acc += 1
        else:
            n_rej += 1
        lam = lam_next(lam, bool(flag), k, h)
        if not np.array_equal(_bits(lam_k), _bits(lam)):
            bad.append("evaluation %d: lambda %r, the recurrence gives %r" % (k, lam_k, lam))
            lam = F32(lam_k)
        if k == 0:
            if not np.array_equal(_bits(run["sigma2_start"]), _bits(F)) and flag:
                bad.append("sigma2_start %r, the first evaluation's F is %r" % (run["sigma2_start"], F))
    if (int(run["accepted"]), int(run["rejected"])) != (n_acc, n_rej) or n_acc + n_rej != n_ev:
        bad.append("counters %d + %d, flags %d + %d of %d" % (run["accepted"], run["rejected"], n_acc, n_rej, n_ev))
    if acc is not None:
        if not np.array_equal(_bits(run["theta"]), _bits(acc)):
            bad.append("returned pose %r, last accepted %r" % (run["theta"], acc))
        if not np.array_equal(_bits(run["sigma2"]), _bits(F_acc)):
            bad.append("sigma2 %r, last accepted F %r" % (run["sigma2"], F_acc))
        if F_acc != tr[:n_ev][tr[:n_ev, 7] > 0][:, 6].min():
            bad.append("the returned pose is not the best trial")
    if not np.array_equal(_bits(run["lam"]), _bits(lam)):
        bad.append("final lambda %r, the recurrence gives %r" % (run["lam"], lam))
    st = int(run["status"])
    if st == 0 and n_ev != iters + 1:
        bad.append("status 0 after %d of %d evaluations" % (n_ev, iters + 1))
    if report is not None and n_ev > 1:
        report(worst[0], worst[2])
    return bad


# ------------------------------------------------------------------------------------------------------------- cases and configurations
TRACE_ITERS = 6
# the hyper-parameters the trace test runs: the defaults; a cap of 2e-7 — a step of an ulp or two, where F often rounds to the SAME fp32
# value (the strict < decides) and every step is capped; and gentle factors (x 2 / x 0.5), under which `tall` rejects trials in a row
CONFIGS = {"default": {}, "tiny_cap": dict(step_cap=2e-7), "gentle": dict(lam_up=2.0, lam_down=0.5)}
_EVALUATORS = {}


def weight_plane(name):
    """(n,) float32 weights in [0.25, 1] of a case, multiples of 2^-10 (so that 4 w is exact)"""
    n = gh.CASES[name][0]
    return (np.floor((0.25 + 0.75 * np.random.default_rng(n).random(n)) * 1024) / 1024).astype(F32)


def scene_pose(oracle, name, b):
    trans, rot = gh.scene(oracle, name)[4:6]
    return np.concatenate([trans[b], rot[b]]).astype(F32)


def scene_evaluator(oracle, name, w=None):
    """theta -> evaluate() on a case's scene (its k/255 image), memoised per pose: the chains of a test visit the same poses again"""
    key = (name, None if w is None else np.asarray(w, F32).tobytes())
    if key not in _EVALUATORS:
        xyz, rgb, img = gh.scene(oracle, name)[:3]
        seen = {}

        def ev(theta):
            k = np.asarray(theta, F32).tobytes()
            if k not in seen:
                seen[k] = evaluate(oracle, (xyz, rgb, img), theta, w)
            return seen[k]
        _EVALUATORS[key] = ev
    return _EVALUATORS[key]


# ------------------------------------------------------------------------------------------------------------------- the free run
FREE_CASES = ("G2", "odd")
FREE_ITERS = 8
FREE_OFFSETS = np.array([[0.05, 0.05, 0.05, 0.03, 0.03, 0.03], [-0.05, 0.05, -0.05, 0.03, -0.03, 0.03]])      # metres, radians
_FREE = {}


def free_centre(oracle, name):
    """(theta, sigma^2) the model converges to from pose 1 of the case's scene: 40 iterations of lm() with the defaults"""
    if ("centre", name) not in _FREE:
        r = lm(scene_evaluator(oracle, name), scene_pose(oracle, name, 1), 40, hyper())
        _FREE["centre", name] = (r["theta"], r["sigma2"])
    return _FREE["centre", name]


def free_starts(oracle, name):
    """the starts of the free-run test: the model's converged pose +- 0.05 m / +- 0.03 rad, in fp32"""
    return [(free_centre(oracle, name)[0].astype(np.float64) + off).astype(F32) for off in FREE_OFFSETS]


def free_yardstick(oracle, name, i):
    """(lo, hi, own): the model's final sigma^2 after FREE_ITERS iterations from start i and from the 12 starts that differ from it by one
    fp32 ulp in one component spans [lo, hi]; own: from the start itself — the model's own sensitivity to its start"""
    if ("yard", name, i) not in _FREE:
        ev, start, h = scene_evaluator(oracle, name), free_starts(oracle, name)[i], hyper()
        finals = [float(lm(ev, start, FREE_ITERS, h)["sigma2"])]
        for c in range(6):
            for to in (-np.inf, np.inf):
                s = start.copy()
                s[c] = np.nextafter(s[c], F32(to))
                finals.append(float(lm(ev, s, FREE_ITERS, h)["sigma2"]))
        _FREE["yard", name, i] = (min(finals), max(finals), finals[0])
    return _FREE["yard", name, i]


def free_bound(lo, hi):
    """hi + FACTOR (hi - lo) + ADDS 2^-24 hi: the model's own spread with grad_helpers' factor, and the kernel's rounding count per sum"""
    return hi + gh.FACTOR * (hi - lo) + ih.ADDS * U * hi
