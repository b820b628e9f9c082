"""The pose information matrix H = sum w m j j^T, b = sum w m l j and the covariance sigma^2 H^-1 (pcl_pose_information; build-defined: the
reference has neither) against a float64 model (tests/info_helpers.py).

CPU: the model is tied to the oracle's own per-point rows, H from j = C a equals C (sum a a^T) C^T, the cases are well conditioned, and
every planted mistake of the model breaks the bound the device is held to.  GPU: one point against the loss kernel's own output (a bound
that counts roundings), the four cases against the model (the per-point gradient bound, propagated), linearity and layout, the covariance
against numpy's inverse of the device's own H, and omniloc_batch's fourth entry."""
import numpy as np
import pytest

import grad_helpers as gh
import info_helpers as ih

gpu = pytest.mark.gpu

FMTS = ("f16", "u8", "f32", "float")
U = ih.U

# which (case, pose, weight scale) catches which planted variant (asserted below).  With 0/1 weights w^2 = w: (a) is planted under
# w = 2 x ok, which the device's model test runs as well.
CATCHERS = {
    "w_squared": [("G2", 0, 2.0), ("tall", 1, 2.0)],
    "masked_in": [("G2", 0, 1.0), ("odd", 1, 1.0), ("tall", 0, 1.0)],
    "pitch_roll": [("G2", 0, 1.0), ("odd", 1, 1.0), ("tiny", 0, 1.0), ("tall", 1, 1.0)],
    "tau_negated": [("G2", 1, 1.0), ("odd", 0, 1.0), ("tiny", 1, 1.0), ("tall", 0, 1.0)],
    "packed_swap": [("G2", 0, 1.0), ("odd", 0, 1.0), ("tiny", 0, 1.0), ("tall", 0, 1.0)],
    "h_over_m": [("G2", 1, 1.0), ("tiny", 0, 1.0)],
    "sigma_s1": [("odd", 0, 1.0), ("tall", 1, 1.0)],
}


# ================================================================================================================ the model (CPU)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_info_model_is_the_oracle(oracle, name):
    """M, S1, S2, H, b of info_model equal the same sums formed from the rows of oracle.sampling_loss(..., visible=identity) to 1e-12
    (relative to sqrt(H_kk H_ll) and sqrt(S2 H_kk): the two add the same products in another order), and H formed as C (sum a a^T) C^T
    from the model's g and tau equals H formed from its j (1e-9: j = C a holds to the rounding of two different float64 formulas)"""
    xyz, rgb, img, imgf, trans, rot = gh.scene(oracle, name)
    for b in range(gh.N_POSES):
        bd = ih.bounds(oracle, name, b)
        sel, w, ref = bd["sel"], bd["w"], bd["ref"]
        loss, count, grad = gh.oracle_rows(oracle, xyz, rgb, img, trans[b], rot[b])
        assert np.array_equal(count[sel], np.ones(sel.sum(), np.int64))
        orc = ih.info_model(dict(grad=grad, loss=loss), sel, w)
        nH = np.sqrt(np.outer(np.diag(ref["H"]), np.diag(ref["H"])))
        assert orc["M"] == ref["M"] == sel.sum()
        assert abs(orc["S1"] - ref["S1"]) <= 1e-12 * ref["S1"] and abs(orc["S2"] - ref["S2"]) <= 1e-12 * ref["S2"]
        assert (np.abs(orc["H"] - ref["H"]) <= 1e-12 * nH).all(), (name, b)
        assert (np.abs(orc["b"] - ref["b"]) <= 1e-12 * np.sqrt(ref["S2"] * np.diag(ref["H"]))).all(), (name, b)
        assert np.linalg.norm(orc["cov"] - ref["cov"]) <= 1e-12 * np.linalg.cond(ref["H"]) * np.linalg.norm(ref["cov"])
        via_a = ih.info_from_a(oracle, bd["m64"], sel, w, rot[b])
        assert (np.abs(via_a["H"] - ref["H"]) <= 1e-9 * nH).all(), (name, b, np.abs(via_a["H"] - ref["H"]).max())
        assert (np.abs(via_a["b"] - ref["b"]) <= 1e-9 * np.sqrt(ref["S2"] * np.diag(ref["H"]))).all(), (name, b)
        assert np.array_equal(ref["H"], ref["H"].T) and (np.linalg.eigvalsh(ref["H"]) > 0).all()


@pytest.mark.parametrize("name", ih.CASES)
def test_the_cases_are_well_conditioned(oracle, name):
    """cond(H) <= 1e3 for every case, pose and image: a covariance compared at cond x 2^-24 means something"""
    for flt in (False, True):
        for b in range(gh.N_POSES):
            ref = ih.bounds(oracle, name, b, flt)["ref"]
            H = ref["H"]
            nH = np.sqrt(np.outer(np.diag(H), np.diag(H)))
            sd = np.sqrt(np.diag(ref["cov"]))
            print("%s flt=%d pose %d: %d pairs, cond %.1f, normalised %.2f, sigma t %.4f..%.4f m, rot %.4f..%.4f rad"
                  % (name, flt, b, int(ref["M"]), np.linalg.cond(H), np.linalg.cond(H / nH), sd[:3].min(), sd[:3].max(), sd[3:].min(), sd[3:].max()))
            assert np.linalg.cond(H) <= 1e3, (name, flt, b)
            assert ref["M"] >= 500


@pytest.mark.parametrize("name", gh.PROBES)
def test_the_term_by_term_sizes_bound_the_models_a(oracle, name):
    """abs_terms >= |a| of the model on every probe (what the counted bounds are relative to), and within 4 x of it wherever a is not a
    cancelling sum: at least half of the entries"""
    m = gh.probe(oracle, name)["m64"]
    a, ah = np.abs(np.concatenate([m["g"], m["tau"]], 1)), ih.abs_terms(m)
    assert np.isfinite(ah).all() and (ah >= a * (1 - 1e-9) - 1e-300).all()
    assert name == "const" or (ah <= 4 * a).mean() >= 0.5


def _variant_result(oracle, variant, name, b, scale):
    bd = ih.bounds(oracle, name, b, False, scale)
    return ih.info_model(bd["m64"], bd["sel"], bd["w"], variant, rot=bd["rot"], oracle=oracle, rgb=bd["rgb"]), bd


def test_the_model_itself_keeps_the_bound(oracle):
    """violations() of the float64 model and of the fp32 model's rows: none (the check does not fire on what it should pass)"""
    for name in ih.CASES:
        for b in range(gh.N_POSES):
            for scale in (1.0, 2.0):
                bd = ih.bounds(oracle, name, b, False, scale)
                assert ih.violations(bd["ref"], bd) == [] and ih.violations(bd["yard"], bd) == [], (name, b, scale)


@pytest.mark.parametrize("variant", list(ih.VARIANTS))
def test_planted_variants_break_the_bound(oracle, variant):
    """each planted mistake of info_model breaks what the device's model test asserts, on every case named for it in CATCHERS"""
    for name, b, scale in CATCHERS[variant]:
        got, bd = _variant_result(oracle, variant, name, b, scale)
        bad = ih.violations(got, bd)
        print("%s on %s pose %d scale %g: %s" % (variant, name, b, scale, bad))
        assert bad, (ih.VARIANTS[variant], name, b, scale)


# ==================================================================================================================== the device
@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rows(out):
    """(H, b, stats, cov) GPU tensors -> one dict of float64 numpy values per pose"""
    H, b, st, cov = (t.cpu().numpy().astype(np.float64) for t in out)
    return [dict(H=H[i], b=b[i], M=st[i, 0], S1=st[i, 1], S2=st[i, 2], sigma2=st[i, 3], status=st[i, 4], cov=cov[i]) for i in range(len(H))]


_CLOUDS, _PANOS = {}, {}


def _pano(ops, oracle, name, fmt):
    from parity_helpers import T
    if (name, fmt) not in _PANOS:
        _, _, img, imgf = gh.scene(oracle, name)[:4]
        _PANOS[name, fmt] = ops.Pano(T(imgf if fmt == "float" else img), fmt="f32" if fmt == "float" else fmt)
    return _PANOS[name, fmt]


def _cloud(ops, oracle, name, sort, weights=None, tag=None):
    from parity_helpers import T
    if (name, sort, tag) not in _CLOUDS:
        xyz, rgb = gh.scene(oracle, name)[:2]
        _CLOUDS[name, sort, tag] = ops.Cloud(T(xyz), T(rgb), sort=sort, weights=None if weights is None else T(weights.astype(np.float32)))
    return _CLOUDS[name, sort, tag]


def _take(m, idx):
    """the rows idx of a model dict"""
    return {key: (v[idx] if isinstance(v, np.ndarray) else v) for key, v in m.items()}


def _abs_chain(oracle, m64, rot):
    """jhat (m,6) = |C| ahat per pair of a probe model (one pose per row), x 1.01; ahat: info_helpers.abs_terms"""
    a = ih.abs_terms(m64)
    out = np.empty_like(a)
    for i in range(len(a)):
        out[i] = np.abs(ih.chain_map(oracle, rot[i])) @ a[i]
    return 1.01 * out


@gpu
@pytest.mark.parametrize("fmt", FMTS[:3])
@pytest.mark.parametrize("name", gh.PROBES)
def test_one_point_against_the_loss_kernel(ops, oracle, name, fmt):
    """a cloud of one point under the poses of a probe class, B odd and B - 1, against ops.sampling_loss(with_grad) on the same cloud and
    poses: M = out[:, 1] exactly, S1 = l exactly, S2 = l^2, H_kl = j_k j_l, b_k = l j_k.

    The bound counts roundings and measures nothing.  The new kernel's a_m (and l) is the loss kernel's single term bit for bit: both are
    0 + v from the same instructions on the same inputs, and every other lane adds zeros.  The kernel rounds once per product,
    A_mn = a_m a_n (1 + e_mn), |e| <= u (w = 1 is an exact factor, 0 + x an exact sum); the chunks' rows are added and the chain rule runs
    in double (2^-53: nothing at this scale); H_kl = fl(sum_mn C_km A_mn C_ln) is one more rounding.  With J = C a in exact arithmetic and
    jhat = |C| ahat:  |H_kl - J_k J_l| <= u jhat_k jhat_l + u |H_kl| <= 2 u jhat_k jhat_l (1 + u).  The loss kernel's j_k = fl(J_k) is one
    rounding each, so |j_k j_l - J_k J_l| <= (2 u + u^2) jhat_k jhat_l.  Together 4 u and terms in u^2: c = 5.
    b_k = fl(sum_m C_km fl(l a_m)): u + u against l J_k, and l j_k is u from it: 3 u and terms in u^2: c = 4.  S1 = fl(1 * l) = l, S2 =
    fl(l * l): c = 1.  jhat is the model's |C| ahat x 1.01 (the device's a is within 1e-3 of the model's on these probes,
    test_point_gradients), with ahat the model's a = [g; tau] evaluated with absolute values term by term (info_helpers.abs_terms): where
    a component cancels exactly in the model — tau_z of a point whose azimuth is clipped — the device keeps the rounding of its terms, and
    |a| itself would bound nothing.
    Masked probes: M = 0, status 1, every sum 0, cov NaN.  The `const` probes (the point's own colour: j = 0): H = 0, status 2, cov NaN."""
    from parity_helpers import T
    k = gh.probe(oracle, name)
    full = len(k["trans"])
    cloud = ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :]))
    pano = ops.Pano(T(k["img"]), fmt=fmt)
    for B in (full, full - 1):
        tr, ro = T(k["trans"][:B]), T(k["rot"][:B])
        out = ops.sampling_loss(cloud, pano, tr, ro).cpu().numpy().astype(np.float64)
        H, b, st, cov = (t.cpu().numpy().astype(np.float64) for t in ops.pose_information(cloud, pano, tr, ro))
        kept = out[:, 1] == 1
        assert np.array_equal(kept, k["m64"]["kept"][:B]) and np.array_equal(st[:, 0], out[:, 1]), (name, fmt, B)
        l, j = out[kept, 0], out[kept, 2:8]
        assert np.array_equal(st[kept, 1], l)
        assert (np.abs(st[kept, 2] - l * l) <= U * l * l + 1e-45).all()
        jh = _abs_chain(oracle, _take(k["m64"], np.nonzero(kept)[0]), k["rot"][:B][kept])
        dH = np.abs(H[kept] - j[:, :, None] * j[:, None, :])
        bH = 5 * U * jh[:, :, None] * jh[:, None, :] + 1e-45
        db = np.abs(b[kept] - l[:, None] * j)
        bb = 4 * U * l[:, None] * jh + 1e-45
        print("%s %s B=%d: %d kept; worst H ratio %.3f, worst b ratio %.3f of the bound" % (name, fmt, B, kept.sum(), (dH / bH).max() if kept.any() else 0,
                                                                                           (db / bb).max() if kept.any() else 0))
        assert (dH <= bH).all(), (name, fmt, B, (dH / bH).max())
        assert (db <= bb).all(), (name, fmt, B, (db / bb).max())
        assert np.array_equal(H, np.swapaxes(H, 1, 2))
        # masked: nothing summed, status 1, cov NaN
        assert (st[~kept, 4] == 1).all() and (H[~kept] == 0).all() and (b[~kept] == 0).all() and (st[~kept, 1:3] == 0).all()
        assert np.isnan(cov[~kept]).all() and np.isnan(st[~kept, 3]).all()
        assert np.isin(st[kept, 4], (0, 2)).all() and np.isfinite(st[kept, :4]).all()
        bad = st[:, 4] != 0
        assert np.isnan(cov[bad]).all() and np.isfinite(cov[~bad]).all()
        if name == "const":
            assert kept.all() and (H == 0).all() and (b == 0).all() and (st[:, 4] == 2).all() and np.isnan(cov).all()
        if name == "black":
            assert (~kept).sum() >= 20


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_against_the_model(ops, oracle, parity, name, fmt):
    """the four cases with 0/1 weights w = ok (no border pair enters a sum), sorted and unsorted packs, both poses (f16 also with
    w = 2 x ok): M the model's count exactly; S1, S2, sigma^2, every entry of H and b within info_helpers.bounds — the per-point bound of
    test_point_gradients and of the residual test, propagated entry by entry, plus ADDS = 13 fp32 roundings per sum (counted at
    info_helpers.ADDS); cov against sigma^2 inv(H) of the device's own H (test_covariance's bound); status 0.


    Achieved on an MI355X, |H - H64| / sqrt(H_kk H_ll), worst entry per case over the formats, packs and poses: G2 1.8e-6, odd 1.8e-6,
    tiny 7.8e-7, tall 4.1e-6 — the fp32 model's own summed H sits at 7.6e-7 to 4.3e-6 there, the bound at 4.0e-5 to 7.5e-2: the device
    uses at most 0.5 % of it at its tightest entry."""
    from parity_helpers import T
    trans, rot = gh.scene(oracle, name)[4:6]
    flt = fmt == "float"
    pano = _pano(ops, oracle, name, fmt)
    for scale in (1.0, 2.0) if fmt == "f16" else (1.0,):
        bds = [ih.bounds(oracle, name, b, flt, scale) for b in range(gh.N_POSES)]
        assert np.array_equal(bds[0]["w"] > 0, gh.case_rule(oracle, name, 0, flt)[2])
        for sort in (True, False):
            got = []
            for b in range(gh.N_POSES):                       # (the decisive pairs, so the weights, differ per pose)
                cloud = _cloud(ops, oracle, name, sort, bds[b]["w"], (flt, b, scale))
                assert (cloud.order is not None) == sort and cloud.weights is not None
                got.append(rows(ops.pose_information(cloud, pano, T(trans[b:b + 1]), T(rot[b:b + 1])))[0])
            for b, (g, bd) in enumerate(zip(got, bds)):
                ref, yard = bd["ref"], bd["yard"]
                nH = np.sqrt(np.outer(np.diag(ref["H"]), np.diag(ref["H"])))
                q = np.abs(g["H"] - ref["H"]) / bd["BH"]
                at = np.unravel_index(np.argmax(q), q.shape)
                tag = "%s %s sort=%d pose %d w=%g" % (name, fmt, sort, b, scale)
                worst = (np.abs(g["H"] - ref["H"]) / nH).max()
                print("%s: M %d (model %d), status %d; |dH|/norm worst %.3e, at the tightest entry %s: %.3e of bound %.3e (fp32 model %.3e); b %.3e of its "
                      "bound; S1 %.3e S2 %.3e sigma2 %.3e of theirs" % (tag, g["M"], ref["M"], g["status"], worst, at, (np.abs(g["H"] - ref["H"]) / nH)[at],
                                                                         (bd["BH"] / nH)[at], (np.abs(yard["H"] - ref["H"]) / nH)[at],
                                                                         (np.abs(g["b"] - ref["b"]) / bd["Bb"]).max(), abs(g["S1"] - ref["S1"]) / bd["BS1"],
                                                                         abs(g["S2"] - ref["S2"]) / bd["BS2"], abs(g["sigma2"] - ref["sigma2"]) / bd["Bsig"]))
                assert g["M"] == ref["M"], tag
                assert g["status"] == 0, tag
                parity(tag + ": H, tightest entry, / sqrt(H_kk H_ll)", (np.abs(g["H"] - ref["H"]) / nH)[at], (bd["BH"] / nH)[at],
                       (np.abs(yard["H"] - ref["H"]) / nH)[at])
                parity(tag + ": H, worst entry, / sqrt(H_kk H_ll)", worst, (bd["BH"] / nH).max(), (np.abs(yard["H"] - ref["H"]) / nH).max())
                nb = np.sqrt(ref["S2"] * np.diag(ref["H"]))
                parity(tag + ": b, worst entry, / sqrt(S2 H_kk)", (np.abs(g["b"] - ref["b"]) / nb).max(), (bd["Bb"] / nb).max(),
                       (np.abs(yard["b"] - ref["b"]) / nb).max())
                assert ih.violations(g, bd) == [], tag


def _probe_single(ops, oracle, name, fmt="f16"):
    from parity_helpers import T
    k = gh.probe(oracle, name)
    B = len(k["trans"]) - 1
    pano = ops.Pano(T(k["img"]), fmt=fmt)
    one = ops.pose_information(ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :])), pano, T(k["trans"][:B]), T(k["rot"][:B]))
    return k, B, pano, one


@gpu
@pytest.mark.parametrize("n", [512, 1024, 1025])
@pytest.mark.parametrize("name", ["fractions", "black"])
def test_copies_of_a_point_sum_to_the_point(ops, oracle, name, n):
    """the probe's point copied n times (every lane, both packed halves; 1024: two steps in one chunk; 1025: two chunks, a ragged last
    step): M = n exactly and H, b, S1, S2 n x the single-point call's.

    Counted: every lane with a point holds the same product v (one rounding, the single-point call's); a lane's second step adds v + v
    (exact); then the two packed halves (1), four DPP steps (4), the rows pairwise (2), the waves pairwise (2): 9 fp32 additions of
    same-signed multiples of v, each within u: |S - n v| <= ((1 + u)^9 - 1) n |v| per packed entry.  The chunks' rows are added and C is
    applied in double, and both calls round their output once: |H_n - n H_1| <= adds n jhat_k jhat_l + u (|H_n| + n |H_1|), likewise b
    with l jhat_k; S1 and S2 have no C: adds n S + 2 u n S.  jhat = |C| ahat of the model x 1.01 (info_helpers.abs_terms)."""
    from parity_helpers import T
    k, B, pano, one = _probe_single(ops, oracle, name)
    cloud = ops.Cloud(T(np.repeat(k["x"][None, :], n, 0)), T(np.repeat(k["rgb"][None, :], n, 0)))
    many = ops.pose_information(cloud, pano, T(k["trans"][:B]), T(k["rot"][:B]))
    H1, b1, s1, _ = (t.cpu().numpy().astype(np.float64) for t in one)
    Hn, bn, sn, _ = (t.cpu().numpy().astype(np.float64) for t in many)
    kept = k["m64"]["kept"][:B]
    assert np.array_equal(s1[:, 0], kept.astype(np.float64)) and np.array_equal(sn[:, 0], n * kept.astype(np.float64))
    assert (sn[~kept, 4] == 1).all() and (Hn[~kept] == 0).all()
    adds = (1 + U) ** 9 - 1
    jh = _abs_chain(oracle, _take(k["m64"], np.nonzero(kept)[0]), k["rot"][:B][kept])
    l = s1[kept, 1]
    dH, bH = np.abs(Hn[kept] - n * H1[kept]), adds * n * jh[:, :, None] * jh[:, None, :] + U * (np.abs(Hn[kept]) + n * np.abs(H1[kept]))
    db, bb = np.abs(bn[kept] - n * b1[kept]), adds * n * l[:, None] * jh + U * (np.abs(bn[kept]) + n * np.abs(b1[kept]))
    print("%s n=%d: worst H %.3f, b %.3f of the bound" % (name, n, (dH / (bH + 1e-300)).max(), (db / (bb + 1e-300)).max()))
    assert (dH <= bH).all() and (db <= bb).all()
    for c in (1, 2):
        assert (np.abs(sn[kept, c] - n * s1[kept, c]) <= (adds + 2 * U) * n * s1[kept, c]).all()


@gpu
def test_a_null_cov_changes_no_bit_of_the_record(ops, oracle):
    """pcl_pose_information with cov = NULL (the header: nullable) on the one-point probe cloud, one pose: the 48-float record of the call
    with a covariance buffer, bit for bit"""
    import torch
    from parity_helpers import T
    k = gh.probe(oracle, "fractions")
    b = int(np.nonzero(k["m64"]["kept"][:len(k["trans"]) - 1])[0][0])
    cloud, pano = ops.Cloud(T(k["x"][None, :]), T(k["rgb"][None, :])), ops.Pano(T(k["img"]), fmt="f16")
    trans, rot = T(k["trans"][b:b + 1]).float().contiguous(), T(k["rot"][b:b + 1]).float().contiguous()
    lib = ops._lib.load()
    nws = lib.pcl_pose_information_workspace_bytes(cloud.n, 1)
    records = []
    for cov in (torch.empty(1, 6, 6, device="cuda"), None):
        info, ws = torch.full((1, 48), float("nan"), device="cuda"), torch.empty(nws, dtype=torch.uint8, device="cuda")
        ops._lib.check(lib.pcl_pose_information(ops._ptr(cloud.data), None, cloud.n, ops._ptr(pano.data), pano.fmt, pano.H, pano.W, ops._ptr(trans),
                                                ops._ptr(rot), 3, 1, ops._ptr(info), ops._ptr(cov), ops._ptr(ws), nws, ops._stream()),
                       "pcl_pose_information")
        records.append(info)
    assert same_bits(records[0], records[1])
    assert float(records[0][0, 42]) == 1.0 and bool(torch.isfinite(records[0]).all())      # M = 1: the point is kept; every slot was written


@gpu
def test_weights_enter_linearly_and_layout_changes_nothing(ops, oracle):
    """on `odd` (2049 points: five steps in three chunks, a ragged last one), f16 texels, both poses in one call:
    weights all 2.0 give exactly twice the unit-weight H, b, S1, S2, M, bit for bit, the same sigma^2, and cov = sigma^2 H^-1 exactly halved
    — a power of two: no other bit of cov changes (the factorisation runs on H scaled by an exact power of two); unit weights give the
    unweighted call's bits; weights all 0 give status 1; two identical calls are bit-identical; pose_stride 16 (a winners tensor) equals
    pose_stride 3 bit for bit; the sorted and the unsorted pack agree within the summation term 2 x ADDS u |C| (sum |a| |a|^T) |C|^T x 1.02
    (the per-point terms do not depend on the slot a point sits in)."""
    import torch
    from parity_helpers import T
    xyz, rgb, img, _, trans, rot = gh.scene(oracle, "odd")
    n = len(xyz)
    pano = _pano(ops, oracle, "odd", "f16")
    tr, ro = T(trans), T(rot)
    plain = ops.pose_information(_cloud(ops, oracle, "odd", True), pano, tr, ro)
    again = ops.pose_information(_cloud(ops, oracle, "odd", True), pano, tr, ro)
    assert all(same_bits(a, b) for a, b in zip(plain, again))
    assert (plain[2][:, 4] == 0).all() and same_bits(plain[3], plain[3].transpose(1, 2)) and same_bits(plain[0], plain[0].transpose(1, 2))
    ones = ops.pose_information(_cloud(ops, oracle, "odd", True, np.ones(n), "ones"), pano, tr, ro)
    assert all(same_bits(a, b) for a, b in zip(plain, ones))
    twos = ops.pose_information(_cloud(ops, oracle, "odd", True, np.full(n, 2.0), "twos"), pano, tr, ro)
    assert same_bits(twos[0], 2 * plain[0]) and same_bits(twos[1], 2 * plain[1]) and same_bits(twos[2][:, :3], 2 * plain[2][:, :3])
    assert same_bits(twos[2][:, 3:], plain[2][:, 3:])
    assert same_bits(twos[3], 0.5 * plain[3])
    zeros = ops.pose_information(_cloud(ops, oracle, "odd", True, np.zeros(n), "zeros"), pano, tr, ro)
    assert (zeros[2][:, 4] == 1).all() and (zeros[2][:, 0] == 0).all() and torch.isnan(zeros[3]).all() and (zeros[0] == 0).all()
    # a winners tensor read in place: t in columns 0-2, yaw / pitch / roll in 13-15
    win = torch.full((2, 16), float("nan"), device="cuda")
    win[:, 0:3], win[:, 13:16] = tr, ro
    at = ops.pose_information_at_winners(_cloud(ops, oracle, "odd", True), pano, win)
    assert all(same_bits(a, b) for a, b in zip(plain, at))
    # the unsorted pack: another summation order only
    uns = ops.pose_information(_cloud(ops, oracle, "odd", False), pano, tr, ro)
    assert same_bits(uns[2][:, 0], plain[2][:, 0])
    for b in range(gh.N_POSES):
        m64 = gh.case_model(oracle, "odd", b)
        kept = m64["kept"]
        a = ih.abs_terms(m64)[kept]
        C = np.abs(ih.chain_map(oracle, rot[b]))
        term = 2 * ih.ADDS * U * 1.02 * (C @ (a.T @ a) @ C.T)
        d = np.abs(uns[0][b].cpu().numpy().astype(np.float64) - plain[0][b].cpu().numpy().astype(np.float64))
        print("odd pose %d: sorted vs unsorted, worst %.3f of the summation term" % (b, (d / term).max()))
        assert (d <= term).all()
        lb = 2 * ih.ADDS * U * 1.02 * (C @ (a * m64["loss"][kept, None]).sum(0))
        assert (np.abs(uns[1][b].cpu().numpy().astype(np.float64) - plain[1][b].cpu().numpy().astype(np.float64)) <= lb).all()


@gpu
@pytest.mark.parametrize("name", ih.CASES)
def test_covariance(ops, oracle, parity, name):
    """the device's cov against sigma^2 inv(H) formed in numpy float64 from the device's own fp32 H and sigma^2, every format, both poses,
    unweighted: ||d|| <= 20 cond(H) 2^-24 ||cov|| (Frobenius; the constant is derived at info_helpers.cov_bound), cov symmetric bit for
    bit, status 0.  An all-black panorama: status 1, M = 0 (not NaN), every sum 0, cov NaN."""
    import torch
    from parity_helpers import T
    trans, rot = gh.scene(oracle, name)[4:6]
    cloud = _cloud(ops, oracle, name, True)
    for fmt in FMTS:
        out = ops.pose_information(cloud, _pano(ops, oracle, name, fmt), T(trans), T(rot))
        assert same_bits(out[3], out[3].transpose(1, 2))
        for b, g in enumerate(rows(out)):
            assert g["status"] == 0 and np.isfinite(g["cov"]).all(), (name, fmt, b)
            want = g["sigma2"] * np.linalg.inv(g["H"])
            cond = np.linalg.cond(g["H"])
            assert cond <= 2e3
            assert abs(g["sigma2"] - g["S2"] / g["M"]) <= 2 * U * g["sigma2"]
            parity("%s %s pose %d: cov vs sigma^2 inv(H), relative Frobenius distance" % (name, fmt, b),
                   np.linalg.norm(g["cov"] - want) / np.linalg.norm(want), ih.cov_bound(g["H"], want) / np.linalg.norm(want), cond * U)
            assert (np.diag(g["cov"]) > 0).all()
    H, W = gh.CASES[name][1:3]
    black = ops.pose_information(cloud, ops.Pano(torch.zeros(H, W, 3, device="cuda"), fmt="f16"), T(trans), T(rot))
    st = black[2].cpu().numpy()
    assert (st[:, 4] == 1).all() and (st[:, :3] == 0).all() and torch.isnan(black[3]).all() and (black[0] == 0).all() and (black[1] == 0).all()


@gpu
def test_omniloc_batch_returns_the_covariance_of_its_winner(ops, oracle):
    """omniloc_batch, 2049 points, 64 x 128, 4 candidates, 6 iterations: with cfg.pose_covariance the first three entries and the written
    back leaves are those of the run without the key, bit for bit, and the fourth is omniloc.pose_covariance at the pose the chain's
    winner row holds (what the first entry returns), bit for bit — plain, with weights=, with robust_iters = [2, 4] (under the chain's
    last weight plane) and with prune_iters / prune_keep."""
    import torch
    from conftest import Cfg
    from parity_helpers import T
    from piccolo_amd import localize, omniloc as po
    xyz, rgb, img, _, trans, rot = gh.scene(oracle, "odd")
    n = len(xyz)
    from piccolo_amd import synth
    t_gt, ypr_gt = synth.gt_pose(gh.SEED)
    trans, rot = synth.start_poses(t_gt, ypr_gt, 4, seed=gh.SEED)
    x, c, im = T(xyz), T(rgb), T(img)
    w = T((0.25 + 0.75 * np.random.default_rng(3).random(n)).astype(np.float32))
    base = dict(num_iter=6, num_input=4, lr=0.1, patience=5, factor=0.9)
    pano, box = po.packed_pano(im, n_points=n), po.quantile_box_of(x, 0.05)

    def batch(weights=None, **kw):
        t, r = T(trans).clone(), T(rot).clone()
        out = po.omniloc_batch(im, x, c, t, r, Cfg(**base, **kw), {}, weights=weights)
        return [o.clone() for o in out], [t.cpu(), r.cpu()]

    def check(engine_win, plane_cloud, weights=None, **kw):
        """engine_win: the (1, 16) winners row of the same chain run through ops; plane_cloud: the cloud whose weights the covariance reads"""
        without, leaves0 = batch(weights, **kw)
        with_cov, leaves1 = batch(weights, pose_covariance=True, **kw)
        assert len(without) == 3 and len(with_cov) == 4
        assert all(same_bits(a, b) for a, b in zip(without, with_cov[:3])) and all(same_bits(a, b) for a, b in zip(leaves0, leaves1))
        win = engine_win.cpu()
        assert same_bits(with_cov[0].reshape(3), win[0, 0:3]) and same_bits(with_cov[1].reshape(9), win[0, 3:12])
        assert same_bits(with_cov[2].reshape(1), win[0, 12:13])
        cov = with_cov[3]
        assert cov.shape == (6, 6) and not cov.is_cuda and cov.dtype == torch.float32 and torch.isfinite(cov).all()
        assert same_bits(cov, cov.t().contiguous()) and (torch.diagonal(cov) > 0).all()
        want = ops.pose_information(plane_cloud, pano, engine_win[:, 0:3].contiguous(), engine_win[:, 13:16].contiguous())[3][0].cpu()
        assert same_bits(cov, want)
        return cov, engine_win

    def engine(cloud):
        return ops.GradientDescent(cloud, pano, T(trans), T(rot), box)
    # plain
    cloud = po.packed_cloud(x, c)
    gd = engine(cloud)
    gd.run(6)
    cov, win = check(gd.winner(1), cloud)
    pc, sig, st = po.pose_covariance(im, x, c, win[:, 0:3].contiguous(), win[:, 13:16].contiguous())
    assert same_bits(pc[0].cpu(), cov) and float(st[0]) == 0 and float(sig[0]) > 0
    ref = localize.refine_image(im, x, c, T(trans).clone(), T(rot).clone(), Cfg(parallel=True, pose_covariance=True, **base))
    assert len(ref) == 4 and same_bits(ref[3], cov)
    assert len(localize.refine_image(im, x, c, T(trans).clone(), T(rot).clone(), Cfg(parallel=True, **base))) == 3
    # the caller's weights
    cw = po.packed_cloud(x, c, w)
    gd = engine(cw)
    gd.run(6)
    cov_w, win = check(gd.winner(1), cw, weights=w)
    assert not same_bits(cov_w, cov)
    assert same_bits(po.pose_covariance(im, x, c, win[:, 0:3].contiguous(), win[:, 13:16].contiguous(), weights=w)[0][0].cpu(), cov_w)
    # the robust chain: under its last weight plane
    gd = engine(cloud)
    gd.run_robust(6, [2, 4], "trunc", 2.5)
    plane = gd._run_weights()
    assert plane is not None and (plane[:n] == 0).any() and cloud.weights is None
    cov_r, _ = check(gd.winner(1), cloud.weighted_view(plane.clone()), robust_iters=[2, 4])
    assert not same_bits(cov_r, cov)
    # a pruned chain: 4 candidates for 3 iterations, the best 2 for the rest
    gd = engine(cloud)
    gd.run(3)
    child, _ = gd.pruned(2)
    child.run(3)
    check(child.winner(1), cloud, prune_iters=3, prune_keep=2)
    with pytest.raises(ValueError, match="pose_covariance"):
        batch(pose_covariance=True, depth_mask=True)
